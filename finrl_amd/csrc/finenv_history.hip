// finenv_history.hip -- MI355X (gfx950): the metrics kernel of every env's episode history
// (finenv_<kind>_history_metrics, include/finenv.h).  The kinds differ in which columns hold the series
// (finenv_host::HistorySeries, filled by each kind's file); the rule is one, series_metrics_of in
// finenv_dev.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finenv.h"
#include "finenv_dev.h"
#include "finenv_host.h"

namespace {

using finenv_host::HistorySeries;

// The three forms a series takes: the value column alone with its pct_change() (stock, crypto, array-state
// stock), the same over value + plus (cash-penalty, stop-loss), the value column with the recorded returns
// (portfolio).  One instantiation each: with the form a run-time branch, the time loops of the first
// two forms ran 25 % and 60 % longer (profiles/history_plumbing.md).
enum SeriesForm { kValue, kSum, kRecorded };

// One lane per env, the time loop strided by E (a wave's accesses are contiguous at every k).  A row
// that lacks one of the `need` flags counts as not armed.  kRecorded: the daily returns are the recorded
// ones, leading 0 included, as the portfolio env's terminal branch takes them: every entry carries one,
// so n_returns is len.  Otherwise they are pct_change() of the values: entry 0 carries none, so
// n_returns is len - 1.
template <SeriesForm FORM>
__global__ void history_metrics_kernel(const HistorySeries p)
{
    const int E = p.E;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const double *v = p.value + e;
    const double *w = FORM == kSum ? p.plus + e : nullptr, *r = FORM == kRecorded ? p.ret + e : nullptr;
    const auto total = [=](int k) {
        if constexpr (FORM == kSum) return v[(size_t)k * E] + w[(size_t)k * E];
        else return v[(size_t)k * E];
    };
    const bool armed = p.need == 0 || (p.flags[e] & p.need) == p.need;
    const int len = armed ? min(p.len[e], p.capacity) : 0;
    double *out = p.out + (size_t)e * FINENV_STOCK_HISTORY_METRICS;
    if constexpr (FORM == kRecorded)
        series_metrics_of(total, len, 0, p.annualization, out, [=](int k) { return r[(size_t)k * E]; });
    else
        series_metrics_of(total, len, 1, p.annualization, out,
                          [=](int k) { return total(k) / total(k - 1) - 1.0; });
}

}  // namespace

namespace finenv_host {

void launch_history_metrics(const HistorySeries &s, hipStream_t stream)
{
    const dim3 grid((s.E + 255) / 256), block(256);
    if (s.ret != nullptr) hipLaunchKernelGGL(history_metrics_kernel<kRecorded>, grid, block, 0, stream, s);
    else if (s.plus != nullptr) hipLaunchKernelGGL(history_metrics_kernel<kSum>, grid, block, 0, stream, s);
    else hipLaunchKernelGGL(history_metrics_kernel<kValue>, grid, block, 0, stream, s);
}

}  // namespace finenv_host
