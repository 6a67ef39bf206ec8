// finenv_twowave_history.hip -- MI355X (gfx950) kernels of the episode history of the cash-penalty and
// stop-loss envs (finenv_{cashpenalty,stoploss}_set_history, include/finenv.h): the reference's
// account_information / actions_memory / transaction_memory of every env's current episode, kept on the
// device: the record and the arm kernel (the metrics kernel is every kind's, finenv_history.hip).  The
// record is a copy of the audit row both step kernels write, so one set of kernels serves both envs;
// finenv_twowave.h declares their argument and launchers and holds the host side.  Time-major layout
// ([k][E], transactions / actions [k][E][N]): a lock-step batch writes whole contiguous rows.
// An object of its own: the two step files keep exactly the kernels they had.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "finenv.h"
#include "finenv_dev.h"
#include "finenv_twowave.h"

namespace {

using finenv_twowave::HistoryArgs;

constexpr int kTwHistThreads = 256;   // envs per block of the record kernel
constexpr int kTwHistBatch = 8;       // elements of a tile each lane has in flight
constexpr int kTwHistNoTx = 1 << 30;  // ks[]: the entry carries no transaction row

// The block's [nenv][N] tile copied flat into entry ks[el] - 1 of dst [k][E][N]: consecutive lanes on
// consecutive elements of the destination (and of each source row; src rows are `pitch` elements
// apart), kTwHistBatch loads in flight before the first store.  skip: bits of ks[] that veto the row.
template <typename T>
__device__ __forceinline__ void tw_history_copy_tile(T *__restrict__ dst, const T *__restrict__ src,
                                                     int pitch, const int *ks, int skip, int nenv,
                                                     int e0, int E, int N, unsigned magicN)
{
    const int total = nenv * N;                       // <= 256 * 32: magicN is exact below 2^16
    for (int f0 = 0; f0 < total; f0 += kTwHistBatch * kTwHistThreads) {
        T v[kTwHistBatch];
#pragma unroll
        for (int j = 0; j < kTwHistBatch; ++j) {
            const int f = min(f0 + j * kTwHistThreads + (int)threadIdx.x, total - 1);
            const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, magicN);
            v[j] = src[(size_t)el * pitch + (f - el * N)];
        }
#pragma unroll
        for (int j = 0; j < kTwHistBatch; ++j) pin(v[j]);
#pragma unroll
        for (int j = 0; j < kTwHistBatch; ++j) {
            const int f = f0 + j * kTwHistThreads + (int)threadIdx.x;
            if (f < total) {
                const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, magicN);
                const int kk = ks[el];
                if ((kk & ~kTwHistNoTx) >= 1 && !(kk & skip))
                    dst[((size_t)((kk & ~kTwHistNoTx) - 1) * E + e0) * N + f] = v[j];
            }
        }
    }
}

// After a step.  Block b owns envs [256 b, 256 b + 256): each lane first decides for its own env whether
// entry k = len[e] is written and publishes k + 1 in LDS (0: no entry), then the whole block copies the
// tile's action rows and, from the audit tile, its transaction rows, and each lane writes its env's
// four scalar columns.  len[e] is read before the barrier and written after it by the lane that owns it.
__global__ __launch_bounds__(kTwHistThreads) void tw_history_record_kernel(const HistoryArgs p)
{
    __shared__ int ks[kTwHistThreads];
    const int E = p.E, N = p.N, cap = p.h.capacity, A = FINENV_AUDIT_HEAD + N;
    const int e0 = blockIdx.x * kTwHistThreads;
    const int e = e0 + (int)threadIdx.x;
    int k1 = 0, ntx = 0, reason = 0;
    bool notx = false;
    double cash = 0.0, asset_value = 0.0, reward = 0.0;
    if (e < E) {
        const double *au = p.audit + (size_t)e * A;               // every load issued together
        const int fl = p.h.flags[e], len = p.h.len[e];
        ntx = p.h.ntx[e];
        const bool done = p.done[e] != 0;
        cash = au[FINENV_AUDIT_BEGIN_CASH];
        asset_value = au[FINENV_AUDIT_ASSET_VALUE];
        reward = au[FINENV_AUDIT_REWARD];
        reason = (int)au[FINENV_AUDIT_FLAGS];
        if ((fl & FINENV_HIST_ARMED) && !(fl & FINENV_HIST_COMPLETE)) {
            int nfl = fl;
            if (reason & FINENV_AUDIT_F_LAST_DATE) {              // :299-301 appends nothing
                nfl |= FINENV_HIST_COMPLETE;
            } else {
                if (len >= cap) {
                    nfl |= FINENV_HIST_OVERFLOW;
                } else {
                    k1 = max(len, 0) + 1;
                    notx = done && (reason & FINENV_AUDIT_F_CASH_SHORTAGE);   // :341-344 returns first
                }
                if (done) nfl |= FINENV_HIST_COMPLETE;
            }
            if (nfl != fl) p.h.flags[e] = nfl;
        }
    }
    ks[threadIdx.x] = k1 | (notx ? kTwHistNoTx : 0);
    __syncthreads();
    const int nenv = min(kTwHistThreads, E - e0);
    if (p.h.actions != nullptr)
        tw_history_copy_tile(p.h.actions, p.actions + (size_t)e0 * N, N, ks, 0, nenv, e0, E, N,
                             p.magicN);
    if (p.h.transactions != nullptr)
        tw_history_copy_tile(p.h.transactions, p.audit + (size_t)e0 * A + FINENV_AUDIT_HEAD, A, ks,
                             kTwHistNoTx, nenv, e0, E, N, p.magicN);
    if (k1 >= 1) {
        const size_t o = (size_t)(k1 - 1) * E + e;
        p.h.cash[o] = cash;
        p.h.asset_value[o] = asset_value;
        p.h.reward[o] = reward;
        p.h.reason[o] = reason;
        p.h.len[e] = k1;
        if (!notx) p.h.ntx[e] = ntx + 1;
    }
}

// What reset() leaves in the lists (:149-154): nothing.  For the envs of the mask: an empty armed record
// that starts on the env's current date and ends with its active window.
__global__ void tw_history_arm_kernel(const HistoryArgs p)
{
    const int E = p.E;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E || (p.mask != nullptr && p.mask[e] == 0)) return;
    p.h.len[e] = 0;
    p.h.ntx[e] = 0;
    p.h.flags[e] = FINENV_HIST_ARMED;
    p.h.start[e] = min(max(p.date_index[e], 0), p.n_days - 1);
    p.h.end[e] = p.win != nullptr ? min(max(p.win[(size_t)3 * E + e], 1), p.n_days) : p.n_days;
}

}  // namespace

namespace finenv_twowave {

void launch_history_record(const HistoryArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(tw_history_record_kernel, dim3((a.E + kTwHistThreads - 1) / kTwHistThreads),
                       dim3(kTwHistThreads), 0, stream, a);
}

void launch_history_arm(const HistoryArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(tw_history_arm_kernel, dim3((a.E + 255) / 256), dim3(256), 0, stream, a);
}

}  // namespace finenv_twowave
