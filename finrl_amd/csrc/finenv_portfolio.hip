// finenv_portfolio.hip -- MI355X (gfx950) kernel + C ABI for the batched StockPortfolioEnv.
//
// Replaces finrl/meta/env_portfolio_allocation/env_portfolio.py step() :125-200,
// reset() :202-220, softmax_normalization :225-229 for E independent envs per launch.
//
// The per-env arithmetic is tiny (softmax over N scores, one N-term fp64 dot product, one
// multiply); the step is a pure HBM write stream: every env receives the day's
// (N+K) x N observation block (4560 B at DOW30 x 8), 95 % of all bytes.  Roofline: HBM.
//   * lane = env for the arithmetic; the [64][N] action tile is read coalesced and
//     transposed through LDS (row stride odd: conflict-free);
//   * one 128-thread block per 64 envs: both waves stream observation rows (32 rows each)
//     with 16-byte stores in row-major order; wave 0 also does the arithmetic and the state;
//   * when all 64 envs sit on the same day (always, in lock-step batches) the template row
//     lives in registers and the row loop holds no load;
//   * per-env episode windows (finenv_portfolio_set_windows) are the WIN instantiation of the step
//     kernel: the terminal test reads the env's window end, a reset goes back to its window start;
//   * the episode history (finenv_portfolio_set_history) is the HIST instantiation: portfolio_return
//     lives in a register of wave 0 and nowhere else, so the record is taken there -- value, return
//     and row by the lane that owns the env, the block's [64][N] weights flat out of the LDS tile
//     (time-major layout: one contiguous run when the block's envs share their entry index).  Wave 1
//     does not take part.  Arming and the metrics are two small kernels off the step path.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "finenv.h"
#include "finenv_dev.h"
#include "finenv_host.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxN = FINENV_PORTFOLIO_MAX_TICKERS;
constexpr int kTileStride = kMaxN + 1;                 // odd row stride (dwords)
constexpr int kThreads = 2 * kWave;
constexpr int kMaxVecChunks = 8;                       // float4 chunks of a row kept in VGPRs

struct PfParams {
    finenv_portfolio_config cfg;
    finenv_portfolio_panel panel;
    finenv_portfolio_state st;
    const float *actions;
    float *obs;
    float *reward;
    uint8_t *done;
    float *term_obs;
    float *weights;
    const uint8_t *mask;
    int32_t auto_reset;
    int32_t D;
    int32_t mode;          // aux kernel: 1 = reset
    uint32_t magicN;
    double *last;          // last-episode block [FINENV_PORTFOLIO_LAST_FIELDS][E] or NULL
    double *stats_out;     // last_episode_stats: [E][3]
    const int32_t *win;    // per-env windows [2][E] (starts, ends) or NULL (finenv_portfolio_set_windows)
    finenv_portfolio_history hist;   // HIST step kernel only (last: the older fields keep their offsets)
};

#define PF(fld) (*at(p.st.f64, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define PI(fld) (*at(p.st.i32, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define PL(fld) (*at(p.last, (unsigned)(fld) * (unsigned)E + (unsigned)e))

// Stream rows [el_lo, el_hi) of the block's observation tile.  row_day: per-lane panel row.
// ROW16: rows on different days take 16-byte loads and stores when D % 4 == 0 (the WIN step kernel, where
// windows put the 64 envs of a block on different days; the other kernels compile as before).
template <bool ROW16 = false>
__device__ __forceinline__ void pf_write_rows(float *__restrict__ dst,
                                              const float *__restrict__ tmpl, int D, int e0,
                                              int el_lo, int el_hi, int row_day,
                                              unsigned long long lane_mask, int lane)
{
    if (el_lo >= el_hi) return;
    unsigned long long sel = lane_mask;
    if (el_hi < 64) sel &= (1ull << el_hi) - 1ull;
    sel &= ~((1ull << el_lo) - 1ull);
    if (sel == 0ull) return;
    const int first = __builtin_ctzll(sel);
    const int rd0 = __builtin_amdgcn_readlane(row_day, first);
    const bool mine = (sel >> lane) & 1ull;
    const bool uniform_row = __all(!mine || row_day == rd0);
    unsigned long long want = (el_hi >= 64 ? ~0ull : (1ull << el_hi) - 1ull) &
                              ~((1ull << el_lo) - 1ull);
    const bool all_rows = sel == want;
    float *const base = dst + (size_t)e0 * D;
    const int n4 = D >> 2;
    const int nchunk4 = (n4 + kWave - 1) / kWave;

    if ((D & 3) == 0 && uniform_row && all_rows && nchunk4 <= kMaxVecChunks) {
        // fast path: 16-byte stores, row-major, template in registers (rows are 16-B aligned
        // because D % 4 == 0 and the tile base is 256-B aligned)
        float4 t[kMaxVecChunks];
#pragma unroll
        for (int j = 0; j < kMaxVecChunks; ++j) {
            const int c4 = j * kWave + lane;
            t[j] = (c4 < n4) ? *at(reinterpret_cast<const float4 *>(tmpl),
                                   (unsigned)(rd0 * n4 + c4))
                             : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float4 *const base4 = reinterpret_cast<float4 *>(base);
#pragma unroll 2
        for (int el = el_lo; el < el_hi; ++el) {
#pragma unroll
            for (int j = 0; j < kMaxVecChunks; ++j) {
                const int c4 = j * kWave + lane;
                if (j < nchunk4 && c4 < n4) *at(base4, (unsigned)(el * n4 + c4)) = t[j];
            }
        }
        return;
    }
    if (ROW16 && (D & 3) == 0) {
        // per-row path with 16-byte template loads and stores (rows 16-B aligned as above)
        const float4 *const tmpl4 = reinterpret_cast<const float4 *>(tmpl);
        float4 *const base4 = reinterpret_cast<float4 *>(base);
        for (int el = el_lo; el < el_hi; ++el) {
            if (!((sel >> el) & 1ull)) continue;
            const int rd = __builtin_amdgcn_readlane(row_day, el);
            for (int c4 = lane; c4 < n4; c4 += kWave)
                *at(base4, (unsigned)(el * n4 + c4)) = *at(tmpl4, (unsigned)(rd * n4 + c4));
        }
        return;
    }
    // general path: per-row template loads (desynchronised days, odd D, masked rows)
    const int nchunk = (D + kWave - 1) / kWave;
    for (int el = el_lo; el < el_hi; ++el) {
        if (!((sel >> el) & 1ull)) continue;
        const int rd = __builtin_amdgcn_readlane(row_day, el);
        for (int k = 0; k < nchunk; ++k) {
            const int col = k * kWave + lane;
            if (col < D) *at(base, (unsigned)(el * D + col)) = *at(tmpl, (unsigned)(rd * D + col));
        }
    }
}

// WIN: the instantiation for batches with per-env episode windows (PfParams::win != NULL).  A template
// parameter so that the no-window kernel compiles exactly as before.
// HIST: the recording instantiation (PfParams::hist attached, finenv_portfolio_set_history; the rule is
// in include/finenv.h).  Wave 0 reads the env's counter and flags beside `day`, writes the env's
// value / return / row where it stores the state, and copies the block's weights out of the LDS tile
// after its own weight loop: no barrier is added, wave 1 goes straight to its observation rows.
template <bool WIN = false, bool HIST = false>
__global__ void __launch_bounds__(kThreads) portfolio_step_kernel(const PfParams p)
{
    __shared__ float tile[kWave * kTileStride];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x >> 6;
    const int E = p.cfg.n_envs, N = p.cfg.n_tickers, D = p.D, T = p.cfg.n_days;
    const int e0 = blockIdx.x * kWave;
    if (e0 >= E) return;
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;

    // both waves: which panel rows this step shows (needs only `day`)
    int day = PI(FINENV_PI_DAY);
    // HIST, wave 0: the env's entry counter and flags, in flight together with `day`
    int hlen = 0, hfl = 0;
    if (HIST && wib == 0 && valid) {
        hlen = *at(p.hist.len, (unsigned)e);
        hfl = *at(p.hist.flags, (unsigned)e);
    }
    const int last_day = WIN ? win_last_day(p.win, E, e, T) : T - 1;         // window end - 1
    const bool term = day >= last_day;                                        // :127
    const int day_next = term ? day : day + 1;
    int start = 0;                                    // the window start (terminal / reset path only)
    if (WIN && __any(term)) start = win_start(p.win, e, T);
    const int row_obs = (term && p.auto_reset) ? start : day_next;           // reset(): window day 0
    const unsigned long long valid_mask = __ballot(valid);
    const unsigned long long term_mask = __ballot(term && valid);

    // stage the action tile (coalesced), split between the two waves
    {
        const float *__restrict__ src = p.actions + (size_t)e0 * N;
        const int total = nenv_w * N;
        for (int f = threadIdx.x; f < total; f += kThreads) {
            const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, p.magicN);
            tile[el * kTileStride + (f - el * N)] = *at(src, (unsigned)f);
        }
    }
    __syncthreads();      // also orders every wave's read of `day` before wave 0 rewrites it

    if (wib == 0) {
        double value = PF(FINENV_PF_VALUE);
        double last_reward = PF(FINENV_PF_LAST_REWARD);
        float *row = tile + lane * kTileStride;
        // HIST: the entry this env records on this step (-1: none).  An armed env (len >= 1; only
        // valid lanes loaded one) whose episode is in progress records unless the step is terminal
        // or the record is full; those two set a flag further down.
        const bool hlive = HIST && hlen >= 1 && !(hfl & FINENV_HIST_COMPLETE);
        const int hk = (hlive && !term && hlen < p.hist.capacity) ? hlen : -1;
        if (!term) {
            // softmax in float32 (:225-229): exp, NumPy pairwise sum order, divide
            float r8[8];
            float den;
            if (N < 8) {
                den = 0.f;
                for (int i = 0; i < N; ++i) {
                    const float ex = expf(row[i]);
                    row[i] = ex;
                    den += ex;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    r8[j] = expf(row[j]);
                    row[j] = r8[j];
                }
                const int full = N - (N & 7);
                for (int i = 8; i < full; i += 8) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float ex = expf(row[i + j]);
                        row[i + j] = ex;
                        r8[j] += ex;
                    }
                }
                den = ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
                for (int i = full; i < N; ++i) {
                    const float ex = expf(row[i]);
                    row[i] = ex;
                    den += ex;
                }
            }
            // portfolio_return = builtin sum(((close_new/close_old) - 1) * weights), :183-185
            double ret = 0.0;
            const unsigned gb = (unsigned)(day * N);
            for (int i = 0; i < N; ++i) {
                const float w = row[i] / den;                                 // :228
                row[i] = w;
                ret = ret + *at(p.panel.gross_ret, gb + (unsigned)i) * (double)w;
            }
            value = value * (1 + ret);                                        // :187-188
            last_reward = value;                                              // :196
            day = day_next;
            if (p.last != nullptr && valid) {  // portfolio_return_memory (:190), as running sums
                PL(FINENV_PL_RUN_SUM) = PL(FINENV_PL_RUN_SUM) + ret;
                PL(FINENV_PL_RUN_SUMSQ) = PL(FINENV_PL_RUN_SUMSQ) + ret * ret;
            }
            if (p.weights != nullptr && valid)
                for (int i = 0; i < N; ++i) *at(p.weights, (unsigned)(e * N + i)) = row[i];
            if (HIST && hk >= 0) {     // :190-193; the time-major slabs are indexed in 64 bits
                const size_t o = (size_t)hk * (size_t)E + (size_t)e;
                p.hist.value[o] = value;
                p.hist.ret[o] = ret;
                p.hist.row[o] = day_next;
                *at(p.hist.len, (unsigned)e) = hk + 1;
            }
        }
        if (HIST) {
            if (hlive && hk < 0) {     // terminal: the record is final; else it is full
                const int nfl = hfl | (term ? FINENV_HIST_COMPLETE : FINENV_HIST_OVERFLOW);
                if (nfl != hfl) *at(p.hist.flags, (unsigned)e) = nfl;   // (an overflowed env: set once)
            }
            const unsigned long long rec = __ballot(hk >= 0);
            if (p.hist.weights != nullptr && rec != 0ull) {
                // actions_memory (:168): the recording envs' rows of the tile hold this step's weights
                // (written by this wave, read back by this wave: no workgroup barrier).  Flat copy,
                // consecutive lanes on consecutive dwords of the block's [nenv][N] slab of weights[k].
                wave_sync();
                const int k0 = __builtin_amdgcn_readlane(hk, __builtin_ctzll(rec));
                const int total = nenv_w * N;                 // <= 64 * 64: magicN is exact
                if (rec == valid_mask && __all(!valid || hk == k0)) {
                    // one k for the whole block (always, in a lock-step batch): one contiguous run
                    float *const dst = p.hist.weights + ((size_t)k0 * (size_t)E + (size_t)e0) * (size_t)N;
                    for (int f = lane; f < total; f += kWave) {
                        const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, p.magicN);
                        *at(dst, (unsigned)f) = tile[el * kTileStride + (f - el * N)];
                    }
                } else {
                    // k differs inside the block (or some envs do not record): each element goes to
                    // its own env's entry; still flat within every env's row
                    for (int f0 = 0; f0 < total; f0 += kWave) {
                        const int f = min(f0 + lane, total - 1);
                        const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, p.magicN);
                        const int kk = __shfl(hk, el);        // every lane takes part
                        if (f0 + lane < total && kk >= 0)
                            p.hist.weights[((size_t)kk * (size_t)E + (size_t)e0) * (size_t)N + (size_t)f] =
                                tile[el * kTileStride + (f - el * N)];
                    }
                }
            }
        }
        if (valid) {
            *at(p.reward, (unsigned)e) = (float)last_reward;
            *at(p.done, (unsigned)e) = term ? 1 : 0;
        }
        if (term && p.last != nullptr && valid) {  // terminal summary :130-155, before any reset
            PL(FINENV_PL_COUNT) = PL(FINENV_PL_COUNT) + 1.0;
            PL(FINENV_PL_BEGIN_VALUE) = p.cfg.initial_amount;                 // asset_memory[0]
            PL(FINENV_PL_END_VALUE) = value;
            PL(FINENV_PL_RET_N) = (double)(day - start + 1);   // the memory's leading 0 (:217) counts
            PL(FINENV_PL_RET_SUM) = PL(FINENV_PL_RUN_SUM);
            PL(FINENV_PL_RET_SUMSQ) = PL(FINENV_PL_RUN_SUMSQ);
            if (p.auto_reset) {
                PL(FINENV_PL_RUN_SUM) = 0.0;
                PL(FINENV_PL_RUN_SUMSQ) = 0.0;
            }
        }
        if (term && p.auto_reset) {                                           // :202-220
            day = start;
            value = p.cfg.initial_amount;
        }
        if (valid) {
            PF(FINENV_PF_VALUE) = value;
            PF(FINENV_PF_LAST_REWARD) = last_reward;
            PI(FINENV_PI_DAY) = day;
        }
    }

    // both waves: observation rows (wave 0: rows [0,32), wave 1: rows [32,64))
    const int el_lo = wib * 32, el_hi = min(nenv_w, el_lo + 32);
    if (term_mask != 0ull && p.term_obs != nullptr)
        pf_write_rows<WIN>(p.term_obs, p.panel.obs_tmpl, D, e0, el_lo, el_hi, day_next, term_mask, lane);
    pf_write_rows<WIN>(p.obs, p.panel.obs_tmpl, D, e0, el_lo, el_hi, row_obs, valid_mask, lane);
}

__global__ void __launch_bounds__(kThreads) portfolio_reset_kernel(const PfParams p)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x >> 6;
    const int E = p.cfg.n_envs, D = p.D, T = p.cfg.n_days;
    const int e0 = blockIdx.x * kWave;
    if (e0 >= E) return;
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;
    const bool sel = valid && (p.mask == nullptr || p.mask[e] != 0);
    const int start = p.win != nullptr ? win_start(p.win, e, T) : 0;        // day 0 of the window
    if (wib == 0 && sel) {
        PF(FINENV_PF_VALUE) = p.cfg.initial_amount;
        PI(FINENV_PI_DAY) = start;
        if (p.last != nullptr) {
            PL(FINENV_PL_RUN_SUM) = 0.0;
            PL(FINENV_PL_RUN_SUMSQ) = 0.0;
        }
    }
    if (p.obs == nullptr) return;
    const int el_lo = wib * 32, el_hi = min(nenv_w, el_lo + 32);
    pf_write_rows(p.obs, p.panel.obs_tmpl, D, e0, el_lo, el_hi, start, __ballot(sel), lane);
}

// {begin, end, Sharpe} of the latched episodes; NaN rows where none has finished yet.
__global__ void portfolio_last_stats_kernel(const PfParams p)
{
    const int E = p.cfg.n_envs;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    double *out = p.stats_out + (size_t)e * 3;
    if (PL(FINENV_PL_COUNT) == 0.0) {
        out[0] = out[1] = out[2] = __builtin_nan("");
        return;
    }
    out[0] = PL(FINENV_PL_BEGIN_VALUE);
    out[1] = PL(FINENV_PL_END_VALUE);
    out[2] = sharpe_from_sums((int)PL(FINENV_PL_RET_N), PL(FINENV_PL_RET_SUM), PL(FINENV_PL_RET_SUMSQ));
}

// -------------------------------------------------------------------------------------
// Episode history, off the step path: arming (the recording itself is the HIST instantiation of the
// step kernel above, the metrics kernel is every kind's, finenv_history.hip).
// -------------------------------------------------------------------------------------
struct PfHistArgs {
    finenv_portfolio_history h;
    finenv_portfolio_state st;
    const uint8_t *mask;          // arm: envs to arm, or NULL = all
    int32_t E, N;
    uint32_t magicN;              // ceil(2^32 / N) for N >= 2
};

constexpr int kArmThreads = 256;      // envs per block of the arm kernel

// What __init__ (:116-123) / reset() (:202-220) leave in the four memories, for the envs of the mask:
// one entry.  value[0] is the env's current portfolio value (the initial amount at the start of an
// episode), ret[0] = 0, row[0] its current panel row, weights[0] the equal-weight row; the block writes
// its [nenv][N] slab of weights[0] flat.
__global__ __launch_bounds__(kArmThreads) void portfolio_history_arm_kernel(const PfHistArgs p)
{
    const int E = p.E, N = p.N;
    const int e0 = blockIdx.x * kArmThreads;
    const int e = e0 + (int)threadIdx.x;
    if (e < E && (p.mask == nullptr || p.mask[e] != 0)) {
        p.h.value[e] = PF(FINENV_PF_VALUE);
        p.h.ret[e] = 0.0;
        p.h.row[e] = PI(FINENV_PI_DAY);
        p.h.len[e] = 1;
        p.h.flags[e] = 0;
    }
    if (p.h.weights == nullptr || e0 >= E) return;
    const int total = min(kArmThreads, E - e0) * N;     // <= 256 * 64: magicN is exact below 2^16
    const float w0 = (float)(1.0 / (double)N);
    for (int f = (int)threadIdx.x; f < total; f += kArmThreads) {
        const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, p.magicN);
        if (p.mask == nullptr || p.mask[e0 + el] != 0) p.h.weights[(size_t)e0 * N + f] = w0;
    }
}

}  // namespace

struct finenv_portfolio : finenv_host::Handle {
    finenv_portfolio_config cfg;
    finenv_portfolio_panel panel;
    finenv_portfolio_state st;
    uint32_t magicN;
    double *last;         // finenv_portfolio_set_last_episode
    int32_t *win;         // finenv_portfolio_set_windows
    int has_hist;         // finenv_portfolio_set_history
    finenv_portfolio_history hist;
};

namespace {
PfParams pf_params(const finenv_portfolio *h)
{
    PfParams p;
    memset(&p, 0, sizeof(p));
    p.cfg = h->cfg;
    p.panel = h->panel;
    p.st = h->st;
    p.D = h->D;
    p.magicN = h->magicN;
    p.last = h->last;
    p.win = h->win;
    if (h->has_hist) p.hist = h->hist;
    return p;
}

PfHistArgs pf_hist_args(const finenv_portfolio *h)
{
    PfHistArgs a;
    memset(&a, 0, sizeof(a));
    a.h = h->hist;
    a.st = h->st;
    a.E = h->cfg.n_envs;
    a.N = h->cfg.n_tickers;
    a.magicN = h->magicN;
    return a;
}

// reset (re)starts episodes: the reference's reset() starts the memories afresh
void launch_history_arm(const finenv_portfolio *h, const uint8_t *mask, hipStream_t stream)
{
    PfHistArgs a = pf_hist_args(h);
    a.mask = mask;
    hipLaunchKernelGGL(portfolio_history_arm_kernel, dim3((a.E + kArmThreads - 1) / kArmThreads),
                       dim3(kArmThreads), 0, stream, a);
}

// the metrics' series: the values, and the RECORDED returns, leading 0 included, as the terminal branch's
// pandas calls take them (:145-152)
finenv_host::HistorySeries history_series(const finenv_portfolio *h)
{
    return {h->hist.value, nullptr, h->hist.ret, h->hist.len, h->hist.flags, 0, h->hist.capacity,
            h->cfg.n_envs};
}

template <bool WIN, bool HIST>
void launch_step(const finenv_portfolio *h, const PfParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL((portfolio_step_kernel<WIN, HIST>), dim3((h->cfg.n_envs + kWave - 1) / kWave),
                       dim3(kThreads), 0, stream, p);
}
}  // namespace

extern "C" {

int finenv_portfolio_create(const finenv_portfolio_config *cfg, finenv_portfolio **out)
{
    if (!cfg || !out) return FINENV_ERR_INVALID;
    *out = nullptr;
    if (cfg->n_envs < 1 || cfg->n_tickers < 1 || cfg->n_tickers > FINENV_PORTFOLIO_MAX_TICKERS ||
        cfg->n_tech < 0 || cfg->n_days < 1)
        return FINENV_ERR_INVALID;
    const long long E = cfg->n_envs, N = cfg->n_tickers, T = cfg->n_days;
    const long long D = (N + cfg->n_tech) * N, lim = (1ll << 32) - 1;
    if (E * 8 * FINENV_PORTFOLIO_F64_FIELDS > lim || T * D * 4 > lim || T * N * 8 > lim ||
        E * N * 4 > lim || 64 * D * 4 > lim)
        return FINENV_ERR_INVALID;
    finenv_portfolio *h = finenv_host::new_handle<finenv_portfolio>(cfg, D);
    if (!h) return FINENV_ERR_NOMEM;
    h->magicN = finenv_host::magic_for(N);
    *out = h;
    return FINENV_OK;
}

void finenv_portfolio_destroy(finenv_portfolio *h) { delete h; }
const char *finenv_portfolio_last_error(const finenv_portfolio *h) { return finenv_host::last_error(h); }
int finenv_portfolio_obs_dim(const finenv_portfolio *h) { return finenv_host::obs_dim(h); }

int finenv_portfolio_bind(finenv_portfolio *h, const finenv_portfolio_panel *panel,
                          const finenv_portfolio_state *st)
{
    if (!h || !panel || !st) return FINENV_ERR_INVALID;
    if (!panel->gross_ret || !panel->obs_tmpl || !st->f64 || !st->i32)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "bind: null pointer");
    return finenv_host::bind(h, panel, st);
}

int finenv_portfolio_reset(finenv_portfolio *h, const uint8_t *mask, float *obs_out, void *stream)
{
    if (const int rc = finenv_host::ready(h, "reset")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    PfParams p = pf_params(h);
    p.mask = mask;
    p.obs = obs_out;
    hipLaunchKernelGGL(portfolio_reset_kernel, dim3((h->cfg.n_envs + kWave - 1) / kWave),
                       dim3(kThreads), 0, (hipStream_t)stream, p);
    if (h->has_hist) launch_history_arm(h, mask, (hipStream_t)stream);   // behind the reset: reads its state
    return finenv_host::check_launch(h, "portfolio_reset");
}

int finenv_portfolio_step(finenv_portfolio *h, const float *actions, float *obs, float *reward,
                          uint8_t *done, float *term_obs, float *weights_out,
                          int32_t auto_reset, void *stream)
{
    if (const int rc = finenv_host::ready(h, "step")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    if (!actions || !obs || !reward || !done)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "step: null actions/obs/reward/done");
    PfParams p = pf_params(h);
    p.actions = actions;
    p.obs = obs;
    p.reward = reward;
    p.done = done;
    p.term_obs = term_obs;
    p.weights = weights_out;
    p.auto_reset = auto_reset;
    const hipStream_t s = (hipStream_t)stream;
    if (p.win != nullptr) {   // per-env windows
        if (h->has_hist) launch_step<true, true>(h, p, s);
        else launch_step<true, false>(h, p, s);
    } else {
        if (h->has_hist) launch_step<false, true>(h, p, s);
        else launch_step<false, false>(h, p, s);
    }
    return finenv_host::check_launch(h, "portfolio_step");
}

int finenv_portfolio_set_last_episode(finenv_portfolio *h, double *last)
{
    if (!h) return FINENV_ERR_INVALID;
    h->last = last;
    return FINENV_OK;
}

int finenv_portfolio_set_windows(finenv_portfolio *h, int32_t *win)
{
    if (!h) return FINENV_ERR_INVALID;
    h->win = win;
    return FINENV_OK;
}

int finenv_portfolio_last_episode_stats(finenv_portfolio *h, double *out, void *stream)
{
    if (!h || !out) return FINENV_ERR_INVALID;
    if (const int rc = finenv_host::ready_last_episode(h, "last_episode_stats")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    PfParams p = pf_params(h);
    p.stats_out = out;
    hipLaunchKernelGGL(portfolio_last_stats_kernel, dim3((h->cfg.n_envs + 255) / 256), dim3(256), 0,
                       (hipStream_t)stream, p);
    return finenv_host::check_launch(h, "portfolio_last_episode_stats");
}

int finenv_portfolio_set_history(finenv_portfolio *h, const finenv_portfolio_history *hist)
{
    if (!h) return FINENV_ERR_INVALID;
    const bool missing = hist && (!hist->value || !hist->ret || !hist->row || !hist->len || !hist->flags);
    return finenv_host::set_history(h, h->hist, h->has_hist, hist,
                                    missing ? "set_history: null value/ret/row/len/flags" : nullptr);
}

int finenv_portfolio_history_arm(finenv_portfolio *h, const uint8_t *mask, void *stream)
{
    return finenv_host::history_arm(h, mask, stream, "portfolio_history_arm", launch_history_arm);
}

int finenv_portfolio_history_metrics(finenv_portfolio *h, double annualization, double *out, void *stream)
{
    return finenv_host::history_metrics(h, annualization, out, stream, "portfolio_history_metrics",
                                        history_series);
}

}  // extern "C"
