// finenv_stock_kernels.inc -- the stock step / aux kernels, compiled once per padded ticker count
// (included by finenv_stock_width.inc inside namespace np32 / np64 / np128 with FINENV_NP,
// FINENV_LOG2NP and FINENV_SORTNET defined).  See finenv_stock.hip for the design notes.

// ---- geometry of this variant (FINENV_NP = padded ticker count: 32, 64 or 128) ---------------
constexpr int kNPad = FINENV_NP;
constexpr int kLog2NPad = FINENV_LOG2NP;
// THE width predicate.  32-wide build (DOW30, the headline): holdings, keys and prices of every ticker
// fit in VGPRs, so the trader stages everything itself ("solo": the streamer depends on nothing but the
// day index and starts streaming ~3 us earlier; an "early release" barrier variant was slower) and
// trades on rank-ordered registers.  Wide builds (64, 128): rolled loops over LDS-resident data, the
// streamer stages holdings and compact price rows for the trader.
constexpr bool kWide = kNPad > 32;
constexpr int kRow = kNPad + 1;                         // LDS row stride in dwords (odd)
constexpr int kAuxWaves = kWide ? 1 : 4;                // waves per block of the aux kernel
constexpr int kLdsPerWave = kWave * kRow;               // >= kNPad * kWave
// |scaled action| saturates here (key packing: kAMax * kNPad + i fits int32); the two values
// include/finenv.h states ("Action domain"), so the 64-wide build does not use its spare bit
constexpr int kAMax = kWide ? 1 << 23 : 1 << 25;
static_assert((long long)kAMax * kNPad + kNPad <= (1ll << 31), "keys must fit int32");
static_assert((1 << kLog2NPad) == kNPad, "NP must be a power of two");

// Batcher network on kNPad statically indexed VGPRs.
__device__ __forceinline__ void sort_keys(int (&k)[kNPad])
{
#define CE(i, j) ce(k[i], k[j]);
#include FINENV_SORTNET
#undef CE
}


// Exact floor(a / d) for d > 0 (what NumPy/CPython `//` returns, env_stocktrading.py:178):
// reciprocal + one Newton step gives a quotient within 1 of the true floor for
// |a/d| < 2^40; the FMA remainder (exact sign) fixes it up.
__device__ __forceinline__ double floordiv_exact(double a, double d)
{
    double x = __builtin_amdgcn_rcp(d);
    x = fma(fma(-d, x, 1.0), x, x);
    double q = floor(a * x);
    const double r = fma(-q, d, a);
    if (r < 0.0) q -= 1.0;
    else if (r >= d) q += 1.0;
    return q;
}

// asset_memory[0] (env_stocktrading.py:364-378): initial=True -> initial_amount +
// np.sum(shares*prices) (NumPy pairwise sum, 8 accumulators for 8 <= n < 128);
// initial=False -> previous cash + builtin sum (sequential from 0).
__device__ __forceinline__ double initial_asset(double cash0, const int (&h)[kNPad],
                                                const double *__restrict__ prow, int N,
                                                bool np_sum)
{
    // Branch-free over the 32 static slots (selects, clamped loads): conditional writes to
    // register arrays would turn them into 32-wide vector PHIs and spill.
    // (panel closes carry the day's untradable flag in their sign bit: |.| everywhere but the trades)
#define PROD(i) ((double)h[i] * fabs(prow[(i) < N ? (i) : 0]))
    double res = 0.0;
    if (!np_sum) {
#pragma unroll
        for (int i = 0; i < kNPad; ++i) {
            const double t = res + fabs(prow[i < N ? i : 0]) * (double)h[i];
            res = (i < N) ? t : res;
        }
    } else if (N < 8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double t = res + PROD(i);
            res = (i < N) ? t : res;
        }
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = PROD(j);
        const int full = N - (N & 7);
#pragma unroll
        for (int i = 8; i < kNPad; ++i) {
            const double t = r[i & 7] + PROD(i);
            r[i & 7] = (i < full) ? t : r[i & 7];
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
#pragma unroll
        for (int i = 8; i < kNPad; ++i) {
            const double t = res + PROD(i);
            res = (i >= full && i < N) ? t : res;
        }
    }
#undef PROD
    return cash0 + res;
}

// Same, with the starting shares in LDS (hcol[i * kWave] = shares of ticker i for this lane)
// and rolled loops: the in-kernel auto-reset path runs once per episode and must not cost
// registers or code size in the step kernel.
__device__ __forceinline__ double initial_asset_lds(double cash0, const int *hcol,
                                                    const double *__restrict__ close,
                                                    unsigned row_base, int N, bool np_sum,
                                                    int hstride = kWave)
{
    auto prod = [&](int i) { return (double)hcol[i * hstride] * fabs(*at(close, row_base + (unsigned)i)); };
    double res = 0.0;
    if (!np_sum) {
        for (int i = 0; i < N; ++i) res = res + fabs(*at(close, row_base + (unsigned)i)) * (double)hcol[i * hstride];
    } else if (N < 8) {
        for (int i = 0; i < N; ++i) res += prod(i);
    } else {
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = prod(j);
        const int full = N - (N & 7);
        for (int i = 8; i < full; i += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += prod(i + j);
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (int i = full; i < N; ++i) res += prod(i);
    }
    return cash0 + res;
}

// Stream observation rows for the envs selected by `lane_mask` (bit el = env e0+el).
//   rows : per-wave LDS, rows[el*kRow + 0] = f32 cash, rows[el*kRow + 1 + i] = f32 holdings_i
//   row_day (per lane el) = panel row whose prices/indicators go into that env's obs.
// Chunk-outer / env-inner; every store instruction writes 256 contiguous bytes.
// Fast path (all selected envs on the same panel row -- always, in lock-step batches): the
// template chunk is loaded ONCE per chunk, so the env loop holds no load and its stores are
// fire-and-forget (a load inside that loop makes hipcc wait vmcnt(0) per iteration, which
// also drains every outstanding store: measured 45 us -> see DESIGN.md).
// `pfn(el, sel)` returns the per-env value of env el: sel = 0 -> f32 cash, sel = 1 + i -> f32
// holdings of ticker i (wherever the caller keeps them in LDS).
// kDesyncCh > 1: this call site gets the 16-byte form of the desynchronised path (the streamer's
// market-data call; one instantiation only -- code size).
template <int kDesyncCh = 1, typename PatchFn>
__device__ __forceinline__ void write_obs_rows_fn(float *__restrict__ dst,
                                                  const float *__restrict__ tmpl, int D, int P, int N,
                                                  int e0, int nenv_w, int row_day,
                                                  unsigned long long lane_mask,
                                                  PatchFn pfn, int lane, int k_lo = 0,
                                                  int k_hi = 1 << 30, int el_lo = 0,
                                                  int el_hi = kWave)
{
    if (lane_mask == 0ull) return;
    const int nchunk = min(k_hi, (D + kWave - 1) / kWave);
    const int first = __builtin_ctzll(lane_mask);
    const int rd0 = __builtin_amdgcn_readlane(row_day, first);
    const bool mine = (lane_mask >> lane) & 1ull;
    const bool uniform_row = __all(!mine || row_day == rd0);
    const unsigned long long full_mask = (nenv_w >= 64) ? ~0ull : ((1ull << nenv_w) - 1ull);
    bool all_rows = lane_mask == full_mask;
    float *const base = dst + (size_t)e0 * P;      // P: row pitch of dst in floats (>= D)

    // Streamer fast path: row-major order (all chunks of a row back to back).  Rows are 1204 B,
    // so a 256-B store chunk straddles 64-B memory segments; writing the neighbouring chunk of
    // the same row immediately lets L2 merge the two halves before they leave for HBM
    // (chunk-major order left them ~64 stores apart: WRITE_SIZE 1.19x the bytes stored).
    // (wide builds keep up to 16 chunk templates in registers: at N = 100 the 11 market-data
    //  chunks used to fall through to the chunk-major path below, whose per-chunk template load
    //  waits for every store of the previous chunk -- vmcnt retires in order)
    // (plain stores on purpose: non-temporal ones were measured 24.7 vs 20.0 us at DOW30 and 70.7 vs 67.8 us
    //  at 100 tickers, same process and buffers -- the rows of the previous step are still in the
    //  Infinity Cache when they are overwritten; profiles/r03_placement.md)
    constexpr int kFast = kNPad <= 64 ? 8 : 16;
    // (dword stores on purpose: 16 bytes per lane -- one store per row and 256 columns -- was measured
    //  slower here, same process and buffers: DOW30 21.3 vs 20.0 us, 100 tickers 71.0 vs 69.9 us; it is
    //  faster in the array-state kernel, whose streamer is slot-bound: profiles/r03_wide_attempts.md)
    if (uniform_row && all_rows && k_lo >= (2 * N) / kWave + 1 && nchunk - k_lo <= kFast) {
        float t[kFast];
#pragma unroll
        for (int j = 0; j < kFast; ++j) {
            const int col = (k_lo + j) * kWave + lane;
            t[j] = (col < D) ? *at(tmpl, (unsigned)(rd0 * D + col)) : 0.0f;
        }
#pragma unroll 2
        for (int el = el_lo; el < min(nenv_w, el_hi); ++el) {
#pragma unroll
            for (int j = 0; j < kFast; ++j) {
                const int col = (k_lo + j) * kWave + lane;
                if (k_lo + j < nchunk && col < D) *at(base, (unsigned)(el * P + col)) = t[j];
            }
        }
        return;
    }

    if (el_lo > 0 || el_hi < kWave) {      // row sub-range on the generic path: fold into the mask
        const unsigned long long hi_m = (el_hi >= 64) ? ~0ull : ((1ull << el_hi) - 1ull);
        lane_mask &= hi_m & ~((1ull << el_lo) - 1ull);
        if (lane_mask == 0ull) return;
        all_rows = false;
    }
    if (!uniform_row) {
        // per-env panel rows (desynchronised days).  A load placed between stores waits until every
        // older store is acknowledged (vmcnt retires in order), so loads and stores alternate in
        // batches of 32 rows.
        constexpr int kRows = 32;
        if constexpr (kDesyncCh > 1) {
            // The streamer's market-data call (columns [k_lo * 64, D) of every row, no per-env value
            // among them): ONE 16-byte-per-lane load and store per row and 256 columns (4-byte
            // aligned addresses; the last quad is shifted back to end at D and rewrites up to
            // three columns of its neighbour with the same values).  A wave keeps at most 64 vector
            // memory operations in flight and retires them in order, ~47 ns per slot at the ~3 us
            // store latency under load: four dword loads + four dword stores per row were 512 slots
            // = 24 us per step for the streamer; this form takes 128.
            typedef float f4 __attribute__((ext_vector_type(4)));
            typedef f4 f4u __attribute__((aligned(4)));
            const int c0 = k_lo * kWave, span = D - c0;
            if (c0 > 2 * N && span >= 4 && k_hi >= (D + kWave - 1) / kWave) {
                const int nq = (span + 3) >> 2;
                for (int q0 = 0; q0 < nq; q0 += kWave) {
                    const bool qa = q0 + lane < nq;
                    const int start = qa ? min(c0 + 4 * (q0 + lane), D - 4) : c0;
                    for (int g = 0; g < nenv_w; g += kRows) {
                        if (((lane_mask >> g) & 0xFFFFFFFFull) == 0ull) continue;
                        f4 t[kRows];
#pragma unroll
                        for (int j = 0; j < kRows; ++j) {
                            const int rd = __builtin_amdgcn_readlane(row_day, min(g + j, nenv_w - 1));
                            t[j] = *reinterpret_cast<const f4u *>(
                                reinterpret_cast<const char *>(tmpl) + (size_t)((unsigned)(rd * D + start) * 4u));
                        }
#pragma unroll
                        for (int j = 0; j < kRows; ++j) pin(t[j]);
#pragma unroll
                        for (int j = 0; j < kRows; ++j) {
                            const int el = g + j;
                            if (el >= nenv_w || !((lane_mask >> el) & 1ull)) continue;
                            if (qa)
                                *reinterpret_cast<f4u *>(reinterpret_cast<char *>(base) +
                                                         (size_t)((unsigned)(el * P + start) * 4u)) = t[j];
                        }
                    }
                }
                return;
            }
        }
        // generic form: 32 rows x 1 chunk of dword loads, then their stores
        for (int k = k_lo; k < nchunk; ++k) {
            const int col = k * kWave + lane;
            const int hidx = col - 1 - N;
            const bool in = col < D;
            const bool patch = in && (col == 0 || (hidx >= 0 && hidx < N));
            const int sel = (col == 0) ? 0 : (patch ? 1 + hidx : 0);
            const bool any_patch = __any(patch);
            for (int g = 0; g < nenv_w; g += kRows) {
                if (((lane_mask >> g) & 0xFFFFFFFFull) == 0ull) continue;
                float t[kRows];
#pragma unroll
                for (int j = 0; j < kRows; ++j) {
                    const int rd = __builtin_amdgcn_readlane(row_day, min(g + j, nenv_w - 1));
                    t[j] = *at(tmpl, (unsigned)(rd * D + (in ? col : 0)));
                }
#pragma unroll
                for (int j = 0; j < kRows; ++j) pin(t[j]);
#pragma unroll
                for (int j = 0; j < kRows; ++j) {
                    const int el = g + j;
                    if (el >= nenv_w || !((lane_mask >> el) & 1ull)) continue;
                    float v = t[j];
                    if (any_patch) {
                        const float pv = pfn(el, sel);
                        v = patch ? pv : v;
                    }
                    if (in) *at(base, (unsigned)(el * P + col)) = v;
                }
            }
        }
        return;
    }
    for (int k = k_lo; k < nchunk; ++k) {
        const int col = k * kWave + lane;
        const bool in = col < D;
        const int hidx = col - 1 - N;
        const bool patch = in && (col == 0 || (hidx >= 0 && hidx < N));
        const int sel = (col == 0) ? 0 : (patch ? 1 + hidx : 0);
        const bool any_patch = __any(patch);
        {
            const float t = in ? *at(tmpl, (unsigned)(rd0 * D + col)) : 0.0f;
            if (all_rows && !any_patch) {
#pragma unroll 8
                for (int el = 0; el < nenv_w; ++el)
                    if (in) *at(base, (unsigned)(el * P + col)) = t;
            } else if (all_rows) {
#pragma unroll 8
                for (int el = 0; el < nenv_w; ++el) {
                    const float pv = pfn(el, sel);
                    if (in) *at(base, (unsigned)(el * P + col)) = patch ? pv : t;
                }
            } else {
                for (int el = 0; el < nenv_w; ++el) {
                    if (!((lane_mask >> el) & 1ull)) continue;
                    const float pv = pfn(el, sel);
                    if (in) *at(base, (unsigned)(el * P + col)) = patch ? pv : t;
                }
            }
        }
    }
}

// rows-in-LDS form: rows[el*kRow + 0] = f32 cash, rows[el*kRow + 1 + i] = f32 holdings_i
template <int kDesyncCh = 1>
__device__ __forceinline__ void write_obs_rows(float *__restrict__ dst,
                                               const float *__restrict__ tmpl, int D, int P, int N,
                                               int e0, int nenv_w, int row_day,
                                               unsigned long long lane_mask,
                                               const float *rows, int lane, int k_lo = 0,
                                               int k_hi = 1 << 30, int el_lo = 0,
                                               int el_hi = kWave)
{
    write_obs_rows_fn<kDesyncCh>(dst, tmpl, D, P, N, e0, nenv_w, row_day, lane_mask,
                      [rows](int el, int sel) { return rows[el * kRow + sel]; }, lane, k_lo, k_hi,
                      el_lo, el_hi);
}

// -------------------------------------------------------------------------------------
// step(): env_stocktrading.py:220-357 (+ DummyVecEnv auto-reset when p.auto_reset)
//
// One block per 64 envs, two specialised waves (lane = env in both) -- three in the lock-step 32-wide
// instantiations, see kThreeWave below: there the sort is the sorter wave's, and so are the last rows of the stream:
//   wave 0 "trader"  : owns the env state; staging (32-wide variant), sort, sells, buys,
//                      assets, reward, state write-back.
//   wave 1 "streamer": streams the market-data part of the observation rows (chunks that
//                      hold no per-env value: 237 of 301 columns at DOW30x8); in the 128-wide
//                      variant it also stages holdings and the price rows for the trader; after
//                      the hand-off barrier it writes the chunk(s) holding cash / holdings.
// At 65,536 envs there is exactly one trader wave per SIMD on the chip and a lone wave issues
// one VALU instruction per ~4 cycles (fp64 ~8) whatever the dependencies, so the trader's
// time is its instruction count; the streamer shares the SIMD and keeps HBM writing
// meanwhile (measured: DESIGN.md "stock_step").
// The observation chunk(s) holding cash / holdings are written after the hand-off barrier, half the
// rows by the streamer (it has finished streaming by then) and half by the trader, which goes on to
// the state write-back.  Measured against the trader writing them alone: 21.5 vs 21.8 us (32-wide),
// and the 128-wide trader is the critical path by far.  This and every alternative named below was a
// compile-time switch once; each was measured in a same-box A/B (DESIGN.md 4.1-4.3) and then removed.
// A new experiment is a `make variant` build run through tools/exp_ab_inproc.py.
// -------------------------------------------------------------------------------------
constexpr int kR1 = kWave * kRow;                 // dwords: act tile / holdings / obs rows
// Price staging.  32-wide variant: f64 [ticker][lane] (per-env day, conflict-free dynamic gather).
// Wide variants: that would be 64 KB and pin the kernel to one block per CU, so they stage compact
// prices -- ONE f64 row [ticker] when the block's 64 envs share the price day (always, in lock-step
// batches) -- and gather from the L1-resident panel row otherwise.
constexpr int kPStride = kWave + 1;              // f64 price rows gathered per env: odd stride (transposed writes)
constexpr int kR2 = kWide ? kNPad * 4 : kNPad * kPStride * 2;   // dwords (compact: current + next row)
constexpr int kR3 = kWave * kRow;                 // dwords: sorted keys [rank][lane] / obs rows
constexpr int kHeadMax = (2 * kNPad) / kWave + 1; // observation chunks holding cash / holdings
constexpr int kR4 = kHeadMax * kWave;             // dwords: their template values (head_park)
constexpr int kR5 = kWide ? 0 : 4;                // dwords: the sorter's "keys are parked" flag (32-wide lock-step)
constexpr int kLdsStep = kR1 + kR2 + kR3 + kR4 + kR5;   // dynamic LDS of the step kernel (dwords)

// One float4 of the [nenv_w][N] action tile -> LDS rows of kRow dwords (magicN = ceil(2^32 / N), N >= 2).
__device__ __forceinline__ void scatter_quad(float *tile, const float4 &v, int idx4, int N, unsigned magicN)
{
    const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int f = 4 * idx4 + u;
        const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, magicN);
        tile[el * kRow + (f - el * N)] = c[u];
    }
}
// the < 4 floats of the tile behind its last whole float4
__device__ __forceinline__ void scatter_leftover(float *tile, const float *__restrict__ act_src, int act_n4,
                                                 int act_total, int N, unsigned magicN, int lane)
{
    for (int f = 4 * act_n4 + lane; f < act_total; f += kWave) {
        const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, magicN);
        tile[el * kRow + (f - el * N)] = *at(act_src, (unsigned)f);
    }
}

// The keys of the canonical order from the transposed action tile: env `lane`, ticker i ->
// trunc(action * hmax) clamped to +-kAMax, -hmax on a turbulent day, 0 where nothing trades; packed with the
// ticker index so that the keys are unique and their order is the stable argsort of the actions (:317).
__device__ __forceinline__ void build_keys(int (&keys)[kNPad], const float *tile, int lane, int N, int hmax,
                                           bool turbulent, bool term)
{
    const float hmaxf = (float)hmax;
#pragma unroll
    for (int i = 0; i < kNPad; ++i) {
        // (slots >= N of the row are padding: read unclamped so every ds_read gets an immediate
        //  offset and issues back to back; the value is discarded by the select below)
        const float x = tile[lane * kRow + i] * hmaxf;                        // f32 mul, :304
        int a = (int)x;                                                       // trunc, :305
        a = max(-kAMax, min(kAMax, a));
        a = turbulent ? -hmax : a;
        a = (term || i >= N) ? 0 : a;                                         // no trading
        keys[i] = a * kNPad + i;          // unique; order == stable argsort(actions), :317
    }
}

// DES: the instantiation for batches whose envs may sit on different days (finenv_stock_set_desync_hint):
// 16-byte row copies in the streamer, row-wise price gather, staging barrier, parked head chunks, head
// rows split in episode-end blocks.  Results never depend on it -- the plain instantiation takes the
// generic per-env paths -- but every one of those paths compiled into the lock-step kernel cost the
// headline 0.1-0.7 us (register allocation, code layout: same-box A/B in DESIGN.md 4.3).
// WIN: the instantiation for batches with per-env episode windows (Params::win != NULL): the terminal
// test reads the env's window end, a reset goes back to its window start.  A template parameter for
// the same reason: the no-window instantiations compile exactly as before.
// kThreeWave<DES>: the lock-step 32-wide kernel runs a third wave per block, the SORTER (role 2).  The keys of
// the canonical order depend on the action row, hmax and two per-lane flags (terminal, turbulent) that come
// with the first round trip -- on nothing the trader's second round trip (cash, holdings, price row) brings.
// So the sorter loads the tile, transposes it, builds and sorts the keys and parks them [rank][lane] in R3
// while the trader's staging loads are in flight, and publishes a flag in LDS; the trader polls the flag and
// reads the keys back by rank.  The sorter then streams the last rows of the block's observation stream and
// ends.  192 threads, 3 waves per SIMD (four blocks per CU as before).  Measured, 65,536 envs x DOW30, same
// process and buffers (profiles/stock_sorter_wave.md): two waves 19.5 us; the sorter without its rows 20.5 --
// the trader reaches its reward 2.8 us sooner, but the streamer, then the long pole, is 1.6 us later --; with
// 16 rows 18.2 - 18.3.
template <bool DES>
constexpr bool kThreeWave = !kWide && !DES;
// s_setprio of the sorter while it holds up its trader (a `make variant EXTRA=-DFINENV_SORTER_PRIO=n` knob)
#ifndef FINENV_SORTER_PRIO
#define FINENV_SORTER_PRIO 3
#endif
// Once it has published the keys the sorter has nothing left to do while the streamer -- the launch's long
// pole as soon as the trader no longer sorts -- still has most of its rows ahead: the sorter writes the
// market-data chunks of the block's last FINENV_SORTER_ROWS rows, the streamer those before them.
#ifndef FINENV_SORTER_ROWS
#define FINENV_SORTER_ROWS 16
#endif
constexpr int kSorterRow0 = kWave - FINENV_SORTER_ROWS;
template <bool DES>
constexpr int kBlockThreads = kThreeWave<DES> ? 3 * kWave : kStepThreads;

// The three-wave kernel's one barrier ahead of the hand-off (see the kernel).  The scheduling fences keep
// hipcc from moving the first use of a loaded value -- and the s_waitcnt it brings -- above the barrier.
__device__ __forceinline__ void flag_barrier()
{
    __builtin_amdgcn_sched_barrier(0);
    lds_barrier();
    __builtin_amdgcn_sched_barrier(0);
}

// The sorter wave (role 2) of the three-wave kernel, lane = env as in the other roles.  term and turbulent are
// per-lane values: the lock-step kernel also steps batches whose envs sit on different days.  Every path ends
// with the flag published -- tail blocks (invalid lanes shadow env e0, their tile rows are never read back by a
// valid lane) and blocks whose envs are all terminal (keys = ticker index) included.
template <bool TURB, bool WIN>
__device__ __forceinline__ void sorter_wave(const Params &p, float *tile, int *ldsk, int *sort_flag,
                                            const float *act_src, int e0, int nenv_w, int e, int lane)
{
    // (act_src is not `__restrict__` on purpose: as a no-alias parameter its loads may sink below the barrier,
    //  into the conditional block of their only use -- one exposed round trip per float4)
    constexpr int role = 2;                          // (STAMP)
    constexpr int kTileLoads = kNPad / 4;            // float4 loads per lane
    const int E = p.cfg.n_envs, N = p.cfg.n_tickers, T = p.cfg.n_days, D = p.D;
    const int act_total = nenv_w * N;
    const int act_n4 = act_total >> 2;
    // the action tile [nenv_w][N] f32 first (16-B coalesced loads), then the two flags' inputs
    float4 av[kTileLoads];
#pragma unroll
    for (int j = 0; j < kTileLoads; ++j) {
        const int idx4 = j * kWave + lane;
        av[j] = reinterpret_cast<const float4 *>(act_src)[(idx4 < act_n4 && !DIAG(8)) ? idx4 : 0];
    }
    const int day = SI(FINENV_SI_DAY);
    const int pd = SI(FINENV_SI_PRICE_DAY);
    const int last_day = WIN ? win_last_day(p.win, E, e, T) : T - 1;         // window end - 1
    double turb = 0.0;
    if (TURB) turb = SF(FINENV_SF_TURBULENCE);
    flag_barrier();                                  // the trader has cleared the flag (see the kernel)
    __builtin_amdgcn_s_setprio(FINENV_SORTER_PRIO);
    STAMP(1);
#pragma unroll
    for (int j = 0; j < kTileLoads; ++j) {
        const int idx4 = j * kWave + lane;
        if (idx4 < act_n4) scatter_quad(tile, av[j], idx4, N, p.magicN);
    }
    scatter_leftover(tile, act_src, act_n4, act_total, N, p.magicN, lane);
    wave_sync();
    STAMP(2);
    int keys[kNPad];
    build_keys(keys, tile, lane, N, p.cfg.hmax, TURB && (turb >= p.cfg.turbulence_threshold), day >= last_day);
    STAMP(3);
    if (!DIAG(4)) sort_keys(keys);
    STAMP(4);
#pragma unroll
    for (int r = 0; r < kNPad; ++r) ldsk[r * kWave + lane] = keys[r];
    // release: the keys, and the last read of the tile in R1, before the flag
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __hip_atomic_store(sort_flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    STAMP(5);
    // ---- second streamer: its share of the rows' market-data chunks (row_obs as in the kernel) ----------
    __builtin_amdgcn_s_setprio(0);
    const bool term = day >= last_day;
    const bool do_reset = term && p.auto_reset != 0;
    int reset_row = 0;
    if (WIN && !p.cfg.reset_quirk && __any(do_reset)) reset_row = win_start(p.win, e, T);
    const int row_obs = do_reset ? (p.cfg.reset_quirk ? pd : reset_row) : (term ? pd : day + 1);
    if (!DIAG(1))
        write_obs_rows(p.obs, p.panel.obs_tmpl, D, p.obs_pitch, N, e0, nenv_w, row_obs, __ballot(lane < nenv_w), tile,
                       lane, (2 * N) / kWave + 1, 1 << 30, kSorterRow0, kWave);
    STAMP(6);
}

template <bool TURB, bool STATS, bool DES = false, bool WIN = false>
__global__ void __launch_bounds__(kBlockThreads<DES>, kWide ? 1 : (kThreeWave<DES> ? 3 : 2))
stock_step_kernel(const Params p)
{
    extern __shared__ __attribute__((aligned(16))) float lds_all[];   // kLdsStep dwords
    constexpr bool kThree = kThreeWave<DES>;
    const int lane = threadIdx.x & (kWave - 1);
    // 0 trader, 1 streamer, 2 sorter (scalar there: no role's registers are live in another's branch)
    const int role = kThree ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;
    float *lds = lds_all;
    int *ldsh = reinterpret_cast<int *>(lds_all);         // [ticker][lane] view of R1
    double *ldsp = reinterpret_cast<double *>(lds_all + kR1);   // [ticker][lane] f64 prices
    int *ldsk = reinterpret_cast<int *>(lds_all + kR1 + kR2);   // [rank][lane] sorted keys
    float *rows = lds_all + kR1 + kR2;                          // later: obs rows [env][kRow]
    float *ldshead = lds_all + kR1 + kR2 + kR3;                 // head-chunk template values
    int *sort_flag = reinterpret_cast<int *>(lds_all + kR1 + kR2 + kR3 + kR4);   // kThree: != 0 = keys parked
    // Action tile [env][kRow]: in R1 for the 32-wide variant (holdings move there from registers
    // once the keys are built); in R3 for the wide ones, whose holdings are staged straight
    // into R1 by the streamer (R3 is free until the sorted keys are parked).
    float *tile = kWide ? rows : lds_all;

    const int E = p.cfg.n_envs, N = p.cfg.n_tickers, D = p.D, T = p.cfg.n_days;
    const int P = p.obs_pitch;                            // row pitch of p.obs in floats (>= D)
    const int e0 = ((int)blockIdx.x + p.block_base) * kWave;
    if (e0 >= E) return;                                  // block-uniform
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;                 // clamped: tail lanes shadow env e0

    STAMP(0);
#ifdef FINENV_DIAG
    if (p.dbg != nullptr && lane == 0) p.dbg[((size_t)blockIdx.x * kStampRoles + role) * 16 + 14] = __builtin_amdgcn_s_memtime();
    // where this wave runs, as in stock_step_wide_kernel: XCC_ID (hwreg 20) in bits 0..7, HW_ID (hwreg 4) above
    if (p.dbg != nullptr && lane == 0)
        p.dbg[((size_t)blockIdx.x * kStampRoles + role) * 16 + 13] =
            (unsigned long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xff) |
            ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 8);
#endif
    // ---- the action tile [nenv_w][N] f32, issued before anything else (16-B coalesced loads): all of
    // it in the trader (32-wide), or half per wave (wide: chunk `it` belongs to wave it & 1) ------
    const float *__restrict__ act_src = p.actions + (size_t)e0 * N;          // 16-B aligned
    const int act_total = nenv_w * N;
    const int act_n4 = act_total >> 2;
    constexpr int kTileLoads = kWide ? kNPad / 8 : kNPad / 4;   // float4 loads per lane
    if constexpr (kThree) {
        if (role == 2) {          // its own loads, barrier and end: nothing of it is live in the other roles
            sorter_wave<TURB, WIN>(p, lds_all, ldsk, sort_flag, act_src, e0, nenv_w, e, lane);
            return;
        }
    }
    float4 av[kTileLoads];
    if (kWide || (!kThree && role == 0)) {
#pragma unroll
        for (int j = 0; j < kTileLoads; ++j) {
            const int idx4 = (kWide ? 2 * j + role : j) * kWave + lane;
            av[j] = reinterpret_cast<const float4 *>(act_src)[(idx4 < act_n4 && !DIAG(8)) ? idx4 : 0];
        }
    }
    // ---- both roles: which panel rows this step touches (needs only day / price_day) -----
    int day = SI(FINENV_SI_DAY);
    int pd = SI(FINENV_SI_PRICE_DAY);
    const int last_day = WIN ? win_last_day(p.win, E, e, T) : T - 1;         // window end - 1
    if constexpr (kThree) {
        // LDS is not initialised at block start, so the sorter's flag is cleared first, behind the ONE workgroup
        // barrier ahead of the hand-off (the sorter meets it in sorter_wave): every wave has issued its first
        // global loads and none has waited yet, so the barrier hides under the first round trip.  The streamer
        // meets no other barrier until it has streamed.  The sorter never meets the hand-off barrier: it ends
        // behind its last store, and a wave that has ended is not counted, so that barrier pairs trader and
        // streamer (and falls once the sorter has ended, should it still be storing then).
        if (role == 0) *sort_flag = 0;
        flag_barrier();
    }
    const bool term = day >= last_day;                                        // :221
    const bool do_reset = term && p.auto_reset != 0;
    const int pd_cur = pd;                            // row held in the current observation
    const int pd_next = term ? pd : day + 1;          // row after the step, before any reset
    int reset_row = 0;                                // the window start (once per episode)
    if (WIN && !p.cfg.reset_quirk && __any(do_reset)) reset_row = win_start(p.win, e, T);
    const int row_obs = do_reset ? (p.cfg.reset_quirk ? pd : reset_row) : pd_next;
    const unsigned long long valid_mask = __ballot(valid);
    const unsigned long long term_mask = __ballot(term && valid);
    const int kpatch = (2 * N) / kWave + 1;           // chunks holding cash/holdings columns
    const int ro_first = __builtin_amdgcn_readfirstlane(row_obs);
    auto head_widx = [N](int col) {                   // column -> index into rows[el * kRow + .]
        const int hidx = col - 1 - N;
        return col == 0 ? 0 : ((hidx >= 0 && hidx < N) ? 1 + hidx : -1);
    };
    const int pd_first = __builtin_amdgcn_readfirstlane(pd_cur);
    const bool uniform_pd = kWide && __all(pd_cur == pd_first);   // same in both waves
    // 32-wide variant, lock-step days: ONE shared price row at the start of the price region
    // (lane i < 32 loads ticker i: one coalesced load instead of 32 wave-uniform ones -- the
    // trader's staging is paced by the number of loads it has in flight under the streamers'
    // store traffic).  Reads go through ldsp[idx * pmul + padd] in either layout.
    const bool shared_row = !kWide && __all(pd_cur == pd_first);
    const bool desync_days = !__all(pd_cur == pd_first);
    const bool gather_rows = DES && !kWide && desync_days;   // row-wise price gather by the streamer (below)
    // Desynchronised days, one head chunk: every env's head chunk comes from its own panel row.  Loading
    // those rows after the hand-off means loads behind a full queue of stores (a ~3 us wait before the
    // first head row can go out).  The streamer -- idle until the staging barrier -- fetches all 64
    // rows' head chunks at the start (16-byte loads, 4 rows per instruction), keeps them while it
    // streams, and parks them in the (by then dead) price region after the hand-off barrier; one more
    // barrier, then both waves write their 32 head rows from LDS.
    const bool park_heads = gather_rows && kpatch == 1 && D >= kWave;
    typedef float hf4 __attribute__((ext_vector_type(4)));
    typedef hf4 hf4u __attribute__((aligned(4)));
    // head rows [el_lo, el_hi) from the parked templates + the (cash, holdings) image in LDS
    auto head_rows_parked = [&](const float *park, const float *img, int el_lo, int el_hi) {
        const int w = head_widx(lane);
        float *const hb = p.obs + (size_t)e0 * P;
        for (int g = el_lo; g < el_hi; g += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float hv = img[(g + j) * kRow + (w >= 0 ? w : 0)];
                const float pv = park[(g + j) * kWave + lane];
                v[j] = w >= 0 ? hv : pv;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (g + j < nenv_w && ((valid_mask >> (g + j)) & 1ull))
                    *at(hb, (unsigned)((g + j) * P + lane)) = v[j];
        }
    };
    const int pmul = shared_row ? 1 : (gather_rows ? kPStride : kWave), padd = shared_row ? 0 : lane;
    const int pn_first = __builtin_amdgcn_readfirstlane(pd_next);
    const bool uniform_next = kWide && __all(pd_next == pn_first);
    STAMP(1);

    // values the trader loads before the barrier (declared here: one barrier call site)
    double cash = 0.0, cost = 0.0, turb = 0.0, last_reward = 0.0, begin = 0.0;
    double st_mean = 0.0, st_m2 = 0.0;
    int trades = 0;
    bool first_step = false;                      // first step of this env's episode (STATS)
    int hreg[kWide ? 1 : kNPad];                  // (wide variants: rolled loops, fewer VGPRs)

    if (role == 0) {
        // ---- trader, part 1: every global load it will ever need, issued up front ----------
        cash = SF(FINENV_SF_CASH);
        begin = SF(FINENV_SF_BEGIN_ASSET);
        cost = SF(FINENV_SF_COST);
        trades = SI(FINENV_SI_TRADES);
        last_reward = SF(FINENV_SF_LAST_REWARD);
        if (TURB) turb = SF(FINENV_SF_TURBULENCE);
        if (STATS) {
            first_step = day == SI(FINENV_SI_START_DAY);
            st_mean = SF(FINENV_SF_RET_SUM);
            st_m2 = SF(FINENV_SF_RET_SUMSQ);
        }
        if (!kWide) {
#pragma unroll
            for (int i = 0; i < kNPad; ++i) {
                // padded slots hold 0 shares: they then add exactly +0.0 to the begin / end asset
                // sums (prices are finite), which saves a select pair per slot in both loops
                const int hv = HOLD(i < N ? i : 0);
                hreg[i] = (i < N) ? hv : 0;
            }
        }
    }
    // (desynchronised instantiation: the STREAMER gathers the 64 price rows -- it idles until the
    //  staging barrier anyway -- and the trader's staging is its own tile / state loads again)
    if (role == ((kWide || gather_rows) ? 1 : 0)) {
        // template values of the head chunks for the end of the step (see head_plan)
        float head_tt[kHeadMax];
        if (!park_heads) head_fetch(head_tt, p.panel.obs_tmpl, D, ro_first, lane, kpatch);
        // ---- stage the current price row in LDS (streamer; the trader in the 32-wide build) -----
        // The day's "untradable" flag of each ticker (first indicator == 1.0, :105/:174) rides
        // in the SIGN BIT of the panel's closes (packed on the host; prices are >= 0 by contract):
        // the trade loops need no mask registers and no bit lookup, the staging no second load.
        if (shared_row) {
            // (tried: SCALAR loads of the row -- constant address space, uniform index, lane 0 parks
            //  it -- to bypass the vector memory pipeline where this wave's loads queue behind four
            //  streamers' stores: 21.3 vs 20.3 us, 32 separate s_load round trips)
            const int i = lane & (kNPad - 1);
            const double pv = *at(p.panel.close, (unsigned)(pd_first * N + (i < N ? i : 0)));
            if (lane < kNPad) ldsp[i] = pv;
        } else if (gather_rows) {
            // every env on its own day: a per-lane load would touch 64 different rows per
            // instruction (2048 scattered 8-byte requests per wave: 10 us of staging under the
            // streamers' store traffic).  Row-wise instead: lane i loads close[day_el][i] for one env
            // per instruction (one 8N-byte segment), all 64 rows in flight, parked transposed
            // [ticker][env] with an odd stride.
            {
                const int l32 = lane & (kNPad - 1);          // (kNPad == 32 here)
                const int li = l32 < N ? l32 : 0;            // padded slots: ticker 0, as below
                double pv[kWave];
#pragma unroll
                for (int j = 0; j < kWave; ++j) {
                    const int de = __builtin_amdgcn_readlane(pd_cur, j);
                    pv[j] = *at(p.panel.close, (unsigned)(de * N + li));
                }
#pragma unroll
                for (int j = 0; j < kWave; ++j)
                    if (lane < kNPad) ldsp[lane * kPStride + j] = pv[j];
            }
        } else if (!kWide) {
            for (int base = 0; base < kNPad; base += 32) {   // 32 loads in flight per batch
                double pv[32];
#pragma unroll
                for (int i = 0; i < 32; ++i)
                    pv[i] = *at(p.panel.close,
                                (unsigned)(pd_cur * N + (base + i < N ? base + i : 0)));
#pragma unroll
                for (int i = 0; i < 32; ++i)
                    ldsp[(base + i) * kWave + lane] = pv[i];
            }
        } else {
            // 128-wide: every staging load of the streamer is issued before the first wait (one
            // exposed round trip instead of five: under load a round trip costs ~3 us).
            int hv[kNPad];
#pragma unroll
            for (int i = 0; i < kNPad; ++i) hv[i] = HOLD(i < N ? i : 0);
            constexpr int kHalves = kNPad / kWave > 0 ? kNPad / kWave : 1;   // (0 in the 32-wide build)
            double pv[kHalves], pn[kHalves];
#pragma unroll
            for (int half = 0; half < kNPad / kWave; ++half) {
                const int i = half * kWave + lane, ic = i < N ? i : 0;
                pv[half] = *at(p.panel.close, (unsigned)(pd_first * N + ic));
                pn[half] = *at(p.panel.close, (unsigned)(pn_first * N + ic));
            }
            // one shared row each (when the block's envs share the day): lane l stages tickers l, l+64
#pragma unroll
            for (int half = 0; half < kNPad / kWave; ++half) {
                const int i = half * kWave + lane;
                ldsp[i] = (i < N) ? pv[half] : 0.0;
                ldsp[kNPad + i] = (i < N) ? fabs(pn[half]) : 0.0;
            }
            // holdings [ticker][lane] (coalesced rows of the state block); the trader, which has
            // no registers to spare for them, used to fetch them 8 at a time inside its
            // begin-asset loop (13 exposed round trips: 24 us of its 68)
#pragma unroll
            for (int i = 0; i < kNPad; ++i) ldsh[i * kWave + lane] = (i < N) ? hv[i] : 0;
        }
        if (!park_heads) head_park(ldshead, head_tt, lane);
    }
    // Desynchronised days (gather_rows): the staging barrier sits HERE for the trader -- its global
    // loads have landed, which is all the streamer has to wait for (the tile transposition below is
    // the trader's own LDS work: 2 us the streamer would otherwise idle through).
    if (gather_rows && role == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        lds_barrier();
    }
    // ---- transpose the action tile into LDS rows (stride 33): half per wave, or all of it in the
    // trader (32-wide) --------------------------------------------------------------------------
    if (kWide || (!kThree && role == 0)) {
#pragma unroll
    for (int j = 0; j < kTileLoads; ++j) {
        const int idx4 = (kWide ? 2 * j + role : j) * kWave + lane;
        if (idx4 < act_n4) {
            const float c[4] = {av[j].x, av[j].y, av[j].z, av[j].w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int f = 4 * idx4 + u;
                const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, p.magicN);
                tile[el * kRow + (f - el * N)] = c[u];
            }
        }
    }
    }
    if (!kThree && role == (kWide ? 1 : 0))
        for (int f = 4 * act_n4 + lane; f < act_total; f += kWave) {          // < 4 leftover floats
            const int el = (N == 1) ? f : (int)__umulhi((unsigned)f, p.magicN);
            tile[el * kRow + (f - el * N)] = *at(act_src, (unsigned)f);
        }
    STAMP(2);
    // (the streamer's head-chunk prefetch: placed here, behind every staging block of the trader, so
    //  that the 64 VGPRs are live in the streamer's branch only)
    hf4 ht[16];
    if (role == 1 && park_heads) {
        const int q = lane & 15, rs = lane >> 4;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int rd = __shfl(row_obs, min(4 * u + rs, nenv_w - 1));
            ht[u] = *reinterpret_cast<const hf4u *>(reinterpret_cast<const char *>(p.panel.obs_tmpl) +
                                                    (size_t)((unsigned)(rd * D + 4 * q) * 4u));
        }
    }
    // Desynchronised days: the trader's staging loads (64 price rows) would otherwise queue behind
    // four streamers' row traffic in the CU's memory pipeline and return when the streaming is
    // over (timeline: staged at 16 us instead of 5, the whole trade serialised behind it).  The
    // streamer waits here until they have landed (the trader met this barrier above).  Otherwise the
    // 32-wide trader staged for itself alone, and the wide builds' waves staged for each other.
    if (gather_rows) {
        if (role == 1) lds_barrier(); else wave_sync();
    } else if (!kWide) {
        wave_sync();
    } else {
        lds_barrier();
    }
    STAMP(3);

    if (role == 1) {
        // ---- streamer, part 2: market-data chunks of the observation rows -------------------
        if (!DIAG(1)) {
            if (term_mask != 0ull && p.term_obs != nullptr)
                write_obs_rows(p.term_obs, p.panel.obs_tmpl, D, D, N, e0, nenv_w, pd_cur,
                               term_mask, lds, lane, kpatch);
            // desynchronised instantiation: 16-byte row copies, this many chunks per batch (1 = dword form)
            constexpr int kDesyncCh = 4;
            // (three-wave form: the block's last rows are the sorter's)
            write_obs_rows<(DES ? kDesyncCh : 1)>(p.obs, p.panel.obs_tmpl, D, P, N, e0, nenv_w, row_obs, valid_mask, lds,
                              lane, kpatch, 1 << 30, 0, kThree ? kSorterRow0 : kWave);
        }
        STAMP(4);
        // ---- streamer, part 3: once the trader has published the (cash, holdings) rows in LDS,
        // write the chunk(s) that contain them; the trader goes on to its state write-back.
        lds_barrier();
        if (park_heads) {
            float *const park = reinterpret_cast<float *>(ldsp);     // (prices are dead by now)
            const int q = lane & 15, rs = lane >> 4;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                *reinterpret_cast<hf4 *>(park + (4 * u + rs) * kWave + 4 * q) = ht[u];
            lds_barrier();
            if (!DIAG(1)) head_rows_parked(park, rows, kWave / 2, kWave);
        } else
        // (episode-end blocks of a desynchronised batch too -- every step has some, and they set
        //  the kernel's duration; rows are final at the barrier.  With lock-step days the trader
        //  keeps them: making the split unconditional cost the headline path 1.3 us)
        if (!DIAG(1) && (term_mask == 0ull || (DES && desync_days))) {
            // rows[el * kRow + w] holds cash (w = 0) and holdings (w = 1 + ticker)
            HeadPlan<kHeadMax> hp;
            head_plan(hp, ldshead, D, row_obs, ro_first, valid_mask, lane, kpatch, head_widx);
            if (hp.uniform)      // rows 32..63 here, rows 0..31 in the trader
                head_store(hp, p.obs, D, P, e0, nenv_w, valid_mask, lane, kWave / 2, kWave,
                           [rows](int el, int w) { return rows[el * kRow + w]; });
            else
                write_obs_rows(p.obs, p.panel.obs_tmpl, D, P, N, e0, nenv_w, row_obs, valid_mask,
                               rows, lane, 0, kpatch, kWave / 2, kWave);
        }
        STAMP(5);
        if (valid) {                           // holdings write-back (final after the barrier)
#pragma unroll 8
            for (int i = 0; i < N; ++i) HOLD(i) = ldsh[i * kWave + lane];
        }
        return;
    }

    // =========================== trader wave only below ===================================
    // 32-wide variant: the trader is the critical path; its instructions win issue arbitration
    // against the streamer wave sharing the SIMD (measured -0.2 us; nothing at 128 wide)
    if (!kWide) __builtin_amdgcn_s_setprio(3);
    // Code-size note: only the key build, the begin-asset sum and the sorting network are
    // unrolled (they need statically indexed VGPRs).  Everything after the sort is a rolled,
    // software-pipelined loop over LDS-resident data: the fully unrolled form was ~55 KB of
    // straight-line code per kernel, i.e. one pass through the whole instruction cache per wave.
    const bool turbulent = TURB && (turb >= p.cfg.turbulence_threshold);      // :308-310
    const int hmax = p.cfg.hmax;
    const float hmaxf = (float)hmax;
    double risk_next = 0.0;
    // (three-wave form, 168 VGPRs: loaded with the next-row prices below -- held from here it is the pair that
    //  no longer fits beside the rank-ordered registers, and its spill waits for the load on the spot)
    if (TURB && !kThree) risk_next = *at(p.panel.risk, (unsigned)pd_next);

    // (the two-wave forms keep their own copy of the tile transposition above and of the key build here:
    //  calling scatter_quad / build_keys from them changed the code of the wide kernels)
    int keys[kNPad];
    if constexpr (!kThree) {
#pragma unroll
    for (int i = 0; i < kNPad; ++i) {
        // (slots >= N of the row are padding: read unclamped so every ds_read gets an immediate
        //  offset and issues back to back; the value is discarded by the select below)
        const float x = tile[lane * kRow + i] * hmaxf;                        // f32 mul, :304
        int a = (int)x;                                                       // trunc, :305
        a = max(-kAMax, min(kAMax, a));
        a = turbulent ? -hmax : a;
        a = (term || i >= N) ? 0 : a;                                         // no trading
        keys[i] = a * kNPad + i;          // unique; order == stable argsort(actions), :317
    }
    }
    wave_sync();

    // signed price of ticker idx for this env (sign bit = untradable flag)
    auto price_signed = [&](int idx) -> double {
        if (!kWide) return ldsp[idx * pmul + padd];
        if (uniform_pd) return ldsp[idx];
        return *at(p.panel.close, (unsigned)(pd_cur * N + min(idx, N - 1)));
    };

    // ---- holdings -> LDS [ticker][lane].  begin_total_asset (:311-314) is NOT recomputed: it is
    // the previous step's end_total_asset bit for bit (the reference evaluates the same expression
    // on the same state list at :344-347 and again at :311-314), carried in the state block
    // (FINENV_SF_BEGIN_ASSET; init / reset evaluate it afresh).  The sum used to cost the trader
    // ~1.3 us of its 15 us critical path (32 LDS reads + 32 fp64 multiply-adds, one wave per SIMD).
    double s = 0.0;
    if constexpr (kThree) {
        // R1 holds the sorter's tile until the keys are parked: poll its flag (acquire) before the
        // holdings go there.  No barrier: the streamer must not stop while it streams.
        STAMP(12);
        while (__hip_atomic_load(sort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
            __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    if (!kWide) {
#pragma unroll
        for (int i = 0; i < kNPad; ++i) ldsh[i * kWave + lane] = hreg[i];
    }
    STAMP(4);

    // ---- canonical order (three-wave form: sorted by the sorter, read back by rank) --------------
    if constexpr (kThree) {
#pragma unroll
        for (int r = 0; r < kNPad; ++r) keys[r] = ldsk[r * kWave + lane];
    } else {
        if (!DIAG(4)) sort_keys(keys);
    }
    const double c_s = p.cfg.sell_cost_pct, c_b = p.cfg.buy_cost_pct;
    const double one_m_cs = 1 - c_s, one_p_cb = 1 + c_b;
    const int *kcol = ldsk + lane;                 // this env's sorted keys, stride kWave
    int *hcol = ldsh + lane;                       // this env's holdings by ticker, stride kWave
    double nreg[kWide ? 1 : kNPad];                // next-row prices, 2 VGPRs per ticker: only where they fit

    if (!kWide) {
        // ======================= 32-wide variant: rank-ordered registers ========================
        // The sorted keys are still in VGPRs, so the (price, holdings) of the ticker at every rank
        // are gathered from LDS with all 64 loads in flight at once -- no load in the trade loops
        // depends on a key any more (the key -> index -> price chain used to set the pace: ~385
        // cycles per rank for a ~100-cycle cash chain).
        double pS[kNPad];
        int hS[kNPad];
#pragma unroll
        for (int r = 0; r < kNPad; ++r) {
            const int idx = keys[r] & (kNPad - 1);
            pS[r] = ldsp[idx * pmul + padd];
            hS[r] = hcol[idx * kWave];
        }
        STAMP(5);
        // ---- sells: most negative first (:317-324, _sell_stock :102-169), straight-line --------
        // Share counts do not depend on cash; cash / cost are summed in rank order.  Ranks that
        // sell nothing add +0.0, which leaves the fp64 sums bit-identical to the reference
        // skipping them.  A ticker is sold OR bought at most once per step.
        if (!DIAG(2)) {
            // Branch-free per rank (sign-bit masks instead of && / if: hipcc turns those into an
            // exec-mask block per rank, ~2x the instructions); ranks are visited in groups of 4
            // and a group is skipped when no lane has a negative key left (sorted ascending).
            int n_sold = 0;
#pragma unroll
            for (int g = 0; g < kNPad; g += 4) {
                if (g >= 8 && !__any(keys[g] < 0)) break;
#pragma unroll
                for (int r = g; r < g + 4; ++r) {
                    const int key = keys[r];
                    const int h = hS[r];
                    const int phi = __double2hiint(pS[r]);     // sign bit = untradable flag
                    // all-ones iff key < 0 and h > 0 and (turbulent ? price != 0 : tradable)
                    // turbulent: sell everything, tradable flag ignored (:139-163); else :105-133
                    int m = (key & -h) >> 31;
                    if (TURB) {
                        const int nz = (fabs(pS[r]) > 0.0) ? -1 : 0;
                        m &= turbulent ? nz : ~(phi >> 31);
                    } else {
                        m &= ~(phi >> 31);
                    }
                    int q = min(-(key >> kLog2NPad), h);
                    if (TURB) q = turbulent ? h : q;
                    q &= m;
                    n_sold -= m;                                                  // :129
                    const double amt = fabs(pS[r]) * (double)q;
                    cash = cash + amt * one_m_cs;                                 // :115-121
                    cost = cost + amt * c_s;                                      // :124-128
                    hcol[(key & (kNPad - 1)) * kWave] = h - q;                    // :123
                }
            }
            trades += n_sold;
        }
        // ---- park keys and the rank-ordered prices (in place: every gather above has issued) ----
#pragma unroll
        for (int r = 0; r < kNPad; ++r) {
            if (!kThree) ldsk[r * kWave + lane] = keys[r];      // (three-wave form: the sorter parked them)
            ldsp[r * kWave + lane] = pS[r];
        }
        STAMP(6);
        // next-row prices for end_total_asset: issued now (the rank-ordered registers are dead), so
        // the loads fly during the buy loop; the fence keeps hipcc from hoisting 64 more live
        // VGPRs above the sell pass
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < kNPad; ++i)
            nreg[i] = *at(p.panel.close, (unsigned)(pd_next * N + (i < N ? i : 0)));
        if (TURB && kThree) risk_next = *at(p.panel.risk, (unsigned)pd_next);
        // ---- buys: largest first (:319, :328-330, _buy_stock :171-213) -------------------------
        // Serial through cash: q = min(a, cash // unit), cash -= p*q*(1+c_b).  Keys and prices are
        // read by RANK (static stride, three ranks ahead); unit price and its refined reciprocal
        // are computed one rank ahead; on the chain `cash // unit` is floor(cash*(1/unit)) clamped
        // to a, made exact by the sign of one FMA remainder:
        //   q0 = min(floor(cash*x), a);  rem = cash - q0*unit (exact sign)
        //   rem < 0 -> q0-1;  rem >= unit and q0 < a -> q0+1;  else q0      == min(a, cash // unit)
        if (!DIAG(2)) {
            const double *pcol = ldsp + lane;
            int key0 = kcol[(kNPad - 1) * kWave], key1 = kcol[(kNPad - 2) * kWave];
            int key2 = kcol[(kNPad - 3) * kWave];
            double p0 = pcol[(kNPad - 1) * kWave], p1 = pcol[(kNPad - 2) * kWave];
            double p2 = pcol[(kNPad - 3) * kWave];
            double u0 = p0 * one_p_cb;                                            // :179
            double x0 = refined_rcp(u0);
#pragma unroll 3
            for (int r = kNPad - 1; r >= 0; --r) {
                if (!__any(key0 >= kNPad)) break;      // sorted: no buys (a >= 1) below this rank
                const int key3 = kcol[max(r - 3, 0) * kWave];
                const double p3 = pcol[max(r - 3, 0) * kWave];
                const double u1 = p1 * one_p_cb;
                const double x1 = refined_rcp(u1);

                const int idx = key0 & (kNPad - 1);
                const int a0 = key0 >> kLog2NPad;
                const double ad = (double)a0;
                const bool ok = key0 >= kNPad && !turbulent && u0 > 0.0;  // u0 <= 0: flagged or no price
                double q0;                                                        // :178-184
                {   // fmin() would first canonicalise `ad` (one more fp64 op on the chain)
                    const double f = floor(cash * x0);
                    asm("v_min_f64 %0, %1, %2" : "=v"(q0) : "v"(f), "v"(ad));
                }
                const double rem = fma(-q0, u0, cash);
                // the +-1 fix-up and the mask run on the integer (fp64 ops cost twice a 32-bit one)
                int qi = (int)q0;
                qi += ((rem >= u0) & (qi < a0)) ? 1 : 0;
                qi -= (rem < 0.0) ? 1 : 0;
                qi = ok ? qi : 0;                          // q = 0 leaves cash / cost bit-identical
                const double amt = p0 * (double)qi;
                cash = cash - amt * one_p_cb;                                     // :185-190
                cost = cost + amt * c_b;                                          // :194-196
                trades += ok ? 1 : 0;                                             // :197
                __hip_atomic_fetch_add(&hcol[idx * kWave], qi, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WAVEFRONT);              // :192
                key0 = key1; key1 = key2; key2 = key3;
                p0 = p1; p1 = p2; p2 = p3; u0 = u1; x0 = x1;
            }
        }
    } else {
    // ======================= 128-wide variant: rolled loops over LDS-resident keys ==============
#pragma unroll
    for (int r = 0; r < kNPad; ++r) ldsk[r * kWave + lane] = keys[r];
    STAMP(5);

    if (uniform_pd) {
        // ---- lock-step days (one shared price row in LDS): the rank-ordered form of the 32-wide
        // variant in register chunks.  Keys of a chunk are read back by rank (static stride),
        // their (price, holdings) gathered with the whole chunk's LDS loads in flight, and the
        // chunk is then processed straight-line -- the rolled loops below expose the
        // key -> index -> price chain on every rank.
        if (!DIAG(2)) {
            int n_sold = 0;
            for (int c = 0; c < kNPad; c += 32) {      // sells: most negative first
                if (!__any(kcol[c * kWave] < 0)) break;            // sorted ascending
                int kk[32], hS[32];
                double pS[32];
#pragma unroll
                for (int r = 0; r < 32; ++r) kk[r] = kcol[(c + r) * kWave];
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    const int idx = kk[r] & (kNPad - 1);
                    pS[r] = ldsp[idx];
                    hS[r] = hcol[idx * kWave];
                }
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    const int key = kk[r];
                    const int h = hS[r];
                    const int phi = __double2hiint(pS[r]);     // sign bit = untradable flag
                    int m = (key & -h) >> 31;   // all-ones iff key < 0 and h > 0 (then the flags)
                    if (TURB) {
                        const int nz = (fabs(pS[r]) > 0.0) ? -1 : 0;
                        m &= turbulent ? nz : ~(phi >> 31);
                    } else {
                        m &= ~(phi >> 31);
                    }
                    int q = min(-(key >> kLog2NPad), h);
                    if (TURB) q = turbulent ? h : q;
                    q &= m;
                    n_sold -= m;                                                  // :129
                    const double amt = fabs(pS[r]) * (double)q;
                    cash = cash + amt * one_m_cs;                                 // :115-121
                    cost = cost + amt * c_s;                                      // :124-128
                    hcol[(key & (kNPad - 1)) * kWave] = h - q;                    // :123
                }
            }
            trades += n_sold;
        }
        STAMP(6);
        if (!DIAG(2)) {
            bool more = true;
            for (int c = kNPad - 16; c >= 0 && more; c -= 16) {    // buys: largest first
                int kk[16];
                double pB[16], uB[16], xB[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) kk[j] = kcol[(c + 15 - j) * kWave];
                if (!__any(kk[0] >= kNPad)) break;                 // sorted: no buys below
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    pB[j] = ldsp[kk[j] & (kNPad - 1)];
                    uB[j] = pB[j] * one_p_cb;                                     // :179
                    xB[j] = refined_rcp(uB[j]);
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int key0 = kk[j];
                    if (!__any(key0 >= kNPad)) { more = false; break; }
                    const int a0 = key0 >> kLog2NPad;
                    const double ad = (double)a0;
                    const bool ok = key0 >= kNPad && !turbulent && uB[j] > 0.0;
                    double q0;                                                    // :178-184
                    {
                        const double f = floor(cash * xB[j]);
                        asm("v_min_f64 %0, %1, %2" : "=v"(q0) : "v"(f), "v"(ad));
                    }
                    const double rem = fma(-q0, uB[j], cash);
                    int qi = (int)q0;
                    qi += ((rem >= uB[j]) & (qi < a0)) ? 1 : 0;
                    qi -= (rem < 0.0) ? 1 : 0;
                    qi = ok ? qi : 0;
                    const double amt = pB[j] * (double)qi;
                    cash = cash - amt * one_p_cb;                                 // :185-190
                    cost = cost + amt * c_b;                                      // :194-196
                    trades += ok ? 1 : 0;                                         // :197
                    __hip_atomic_fetch_add(&hcol[(key0 & (kNPad - 1)) * kWave], qi,
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
                }
            }
        }
    } else {
    // ---- sells: most negative first (:317-324, _sell_stock :102-169) ---------------------------
    // Two-deep software pipeline: the key of rank r+2 and the (holdings, price) of rank r+1 are in
    // flight while rank r is applied.
    if (!DIAG(2)) {
        int key0 = kcol[0];
        int key1 = kcol[1 * kWave];
        int h0 = hcol[(key0 & (kNPad - 1)) * kWave];
        double q0p = price_signed(key0 & (kNPad - 1));
        int n_sold = 0;
#pragma unroll 2
        for (int r = 0; r < kNPad; ++r) {
            if (!__any(key0 < 0)) break;               // sorted: no sells beyond this rank
            const int key2 = kcol[min(r + 2, kNPad - 1) * kWave];
            const int i1 = key1 & (kNPad - 1);
            const int h1 = hcol[i1 * kWave];
            const double p1 = price_signed(i1);

            const int idx = key0 & (kNPad - 1);
            const int a = key0 >> kLog2NPad;
            const bool ok = key0 < 0 && h0 > 0 &&
                            (turbulent ? (fabs(q0p) > 0.0) : !__builtin_signbit(q0p));
            const int q = ok ? (turbulent ? h0 : min(-a, h0)) : 0;
            hcol[idx * kWave] = h0 - q;                                       // :123
            n_sold += ok ? 1 : 0;                                             // :129
            const double amt = fabs(q0p) * (double)q;
            cash = cash + amt * one_m_cs;                                     // :115-121
            cost = cost + amt * c_s;                                          // :124-128
            key0 = key1; key1 = key2; h0 = h1; q0p = p1;
        }
        trades += n_sold;
    }
    STAMP(6);

    // ---- buys (same arithmetic as the 32-wide variant; prices gathered per rank) ---------------
    if (!DIAG(2)) {
        int key0 = kcol[(kNPad - 1) * kWave];
        int key1 = kcol[(kNPad - 2) * kWave];
        double p0 = price_signed(key0 & (kNPad - 1));
        double u0 = p0 * one_p_cb;                                            // :179
        double x0 = refined_rcp(u0);
#pragma unroll 2
        for (int r = kNPad - 1; r >= 0; --r) {
            if (!__any(key0 >= kNPad)) break;          // sorted: no buys (a >= 1) below this rank
            const int key2 = kcol[max(r - 2, 0) * kWave];
            const double p1 = price_signed(key1 & (kNPad - 1));
            const double u1 = p1 * one_p_cb;
            const double x1 = refined_rcp(u1);

            const int idx = key0 & (kNPad - 1);
            const double ad = (double)(key0 >> kLog2NPad);
            const bool ok = key0 >= kNPad && !turbulent && u0 > 0.0;     // u0 <= 0: flagged (sign) or no price
            const double q0 = fmin(floor(cash * x0), ad);                     // :178-184
            const double rem = fma(-q0, u0, cash);
            const double adj = ((rem < 0.0) ? -1.0 : 0.0) + ((rem >= u0 && q0 < ad) ? 1.0 : 0.0);
            const double qd = ok ? q0 + adj : 0.0;     // q = 0 leaves cash / cost bit-identical
            const double amt = p0 * qd;
            cash = cash - amt * one_p_cb;                                     // :185-190
            cost = cost + amt * c_b;                                          // :194-196
            trades += ok ? 1 : 0;                                             // :197
            // ds_add (no return): a plain `+=` is an LDS read-modify-write whose wait stalls
            // every iteration of this serial loop for a full LDS round trip
            __hip_atomic_fetch_add(&hcol[idx * kWave], (int)qd, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WAVEFRONT);              // :192
            key0 = key1; key1 = key2; p0 = p1; u0 = u1; x0 = x1;
        }
    }
    }
    }
    STAMP(7);

    // ---- day += 1, new row, end_total_asset (:335-347); obs rows -> LDS (keys are dead) -------
    if (!term) {
        day += 1;
        pd = day;
        if (TURB) turb = risk_next;
    }
    wave_sync();
    s = 0.0;
    if (!kWide) {
#pragma unroll
        for (int i = 0; i < kNPad; ++i) {
            const int h = hcol[i * kWave];
            s = s + fabs(nreg[i]) * (double)h;     // padded slots: h == 0
            rows[lane * kRow + 1 + i] = (float)h;   // slots > N: padding, never read
        }
    } else {
        if (uniform_next) {                      // next row staged in LDS by the streamer
#pragma unroll 8
            for (int i = 0; i < N; ++i) {
                const int h = hcol[i * kWave];
                s = s + ldsp[kNPad + i] * (double)h;
                rows[lane * kRow + 1 + i] = (float)h;
            }
        } else {
            const unsigned nb = (unsigned)(pd_next * N);
#pragma unroll 8
            for (int i = 0; i < N; ++i) {
                const int h = hcol[i * kWave];
                s = s + fabs(*at(p.panel.close, nb + (unsigned)i)) * (double)h;
                rows[lane * kRow + 1 + i] = (float)h;
            }
        }
    }
    rows[lane * kRow] = (float)cash;
    const double end = cash + s;
    double end_carry = term ? begin : end;          // the next step's begin asset
    STAMP(8);
    if (!term) last_reward = (end - begin) * p.cfg.reward_scaling;            // :350-352
    if (valid) {
        *at(p.reward, (unsigned)e) = (float)last_reward;
        *at(p.done, (unsigned)e) = term ? 1 : 0;
    }
    if (p.realised != nullptr && valid) {    // traded shares == holdings delta (:324, :330)
        for (int i = 0; i < N; ++i)
            *at(p.realised, (unsigned)(e * N + i)) = hcol[i * kWave] - HOLD(i);
    }
    STAMP(9);
    wave_sync();

    // ---- terminal observation; auto-reset (once per episode, wave-uniform) ---------------------
    int episode_inc = 0;
    if (term_mask != 0ull) {
        // last-episode block: before the auto-reset below rewrites the state.  At `term` the end
        // asset equals the carried begin asset (no trade, same row); the STATS kernels keep `end`
        // live for the Sharpe sums anyway, the others hand over end_carry (live until write-back).
        double *const last = last_block();       // (not p.last: see last_block)
        if (last != nullptr && term && valid) latch_last_episode(p, last, E, e, STATS ? end : end_carry);
        if (p.term_obs != nullptr)
            write_obs_rows(p.term_obs, p.panel.obs_tmpl, D, D, N, e0, nenv_w, pd_cur, term_mask,
                           rows, lane, 0, kpatch);
        if (p.auto_reset) {                  // reset(), :359-393
            wave_sync();
            if (term) {
                pd = row_obs;
                cash = SF(FINENV_SF_CASH0);
                for (int i = 0; i < N; ++i) {
                    const int v = SH0(i);
                    hcol[i * kWave] = v;
                    rows[lane * kRow + 1 + i] = (float)v;
                }
                rows[lane * kRow] = (float)cash;
                const double a0 = initial_asset_lds(cash, hcol, p.panel.close, (unsigned)(pd * N),
                                                    N, p.cfg.initial != 0);
                if (p.cfg.single_ticker && p.cfg.initial) {   // single stock: `[0] * stock_dim` shares
                    hcol[0] = 0;                              // (:415-422); asset_memory[0] above
                    rows[lane * kRow + 1] = 0.0f;             // still counts num_stock_shares (:364-370)
                }
                // begin asset of the episode's first step: sequential order (:311-314)
                end_carry = initial_asset_lds(cash, hcol, p.panel.close, (unsigned)(pd * N), N, false);
                day = WIN ? win_start(p.win, e, T) : 0;                       // day 0 of the window
                if (valid) {
                    store_episode_start(p, E, e, a0, day);
                }
                turb = 0.0;
                cost = 0.0;
                trades = 0;
                episode_inc = 1;
            }
            wave_sync();
        }
    }

    // ---- the observation chunk(s) holding cash / holdings (:342 / :453-478): after this barrier
    // (rows are final) the streamer writes rows 32..63 and the trader rows 0..31 (its template loads
    // go out before its state stores) ---------------------------------------------------------------
    lds_barrier();
    if (park_heads) lds_barrier();            // the streamer has parked every row's head chunk
    HeadPlan<kHeadMax> hpt;
    const bool split_head = term_mask == 0ull || (DES && desync_days);
    if (split_head && !park_heads)
        head_plan(hpt, ldshead, D, row_obs, ro_first, valid_mask, lane, kpatch, head_widx);
    if (!DIAG(1) && !split_head && !park_heads)
        write_obs_rows(p.obs, p.panel.obs_tmpl, D, P, N, e0, nenv_w, row_obs, valid_mask, rows, lane,
                       0, kpatch);
    STAMP(10);

    // ---- the Sharpe sums, placed after the observation stores (nothing waits on them but their own
    // write-back); then the state write-back ------------------------------------------------------------
    if (STATS && !term) store_sharpe_sums(p, E, e, valid, begin, end, first_step, st_mean, st_m2);
    if (valid) store_trader<TURB>(p, E, e, cash, end_carry, cost, trades, day, pd, last_reward, turb, episode_inc);
    if (park_heads) {
        if (!DIAG(1)) head_rows_parked(reinterpret_cast<const float *>(ldsp), rows, 0, kWave / 2);
    } else if (split_head && !DIAG(1)) {
        if (hpt.uniform)
            head_store(hpt, p.obs, D, P, e0, nenv_w, valid_mask, lane, 0, kWave / 2,
                       [rows](int el, int w) { return rows[el * kRow + w]; });
        else
            write_obs_rows(p.obs, p.panel.obs_tmpl, D, P, N, e0, nenv_w, row_obs, valid_mask, rows, lane,
                           0, kpatch, 0, kWave / 2);
    }
    STAMP(11);
    stamp_wave_end(p, lane, role);
}

// -------------------------------------------------------------------------------------
// reset() :359-393 (masked), __init__ state :64-91, render() :395-396
// mode 0 = init (no obs), 1 = reset (masked, obs for reset envs), 2 = observe only,
// mode 3 = refresh: re-evaluate the carried begin asset from the current cash / holdings / row
// -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWave *kAuxWaves) stock_aux_kernel(const Params p, int mode)
{
    __shared__ float lds_all[kAuxWaves * kLdsPerWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x >> 6;
    float *lds = lds_all + wib * kLdsPerWave;
    const int E = p.cfg.n_envs, N = p.cfg.n_tickers, D = p.D, P = p.obs_pitch, T = p.cfg.n_days;
    const int e0 = (blockIdx.x * kAuxWaves + wib) * kWave;
    if (e0 >= E) return;
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;

    int hf[kNPad];
    double cash;
    int pd, start = 0;
    bool sel = valid;
    if (mode >= 2) {
        cash = SF(FINENV_SF_CASH);
        pd = SI(FINENV_SI_PRICE_DAY);
#pragma unroll
        for (int i = 0; i < kNPad; ++i) {
            const int v = HOLD(i < N ? i : 0);
            hf[i] = (i < N) ? v : 0;
        }
        if (mode == 3) {      // cash + builtin sum(close * shares) of the row held now (:311-314)
            const double b0 = initial_asset(cash, hf, p.panel.close + (size_t)pd * N, N, false);
            if (valid) SF(FINENV_SF_BEGIN_ASSET) = b0;
            return;
        }
    } else {
        if (mode == 1 && p.mask != nullptr) sel = valid && p.mask[e] != 0;
        // first day of the episode: day0 / 0, counted from the env's window start when windows are set
        const int w0 = p.win != nullptr ? win_start(p.win, e, T) : 0;
        start = mode == 0 ? min(w0 + p.day0, T - 1) : w0;
        if (mode == 0) pd = start;
        else pd = p.cfg.reset_quirk ? SI(FINENV_SI_PRICE_DAY) : start;
        cash = SF(FINENV_SF_CASH0);
#pragma unroll
        for (int i = 0; i < kNPad; ++i) {
            const int v = SH0(i < N ? i : 0);
            hf[i] = (i < N) ? v : 0;
        }
        const double a0 =
            initial_asset(cash, hf, p.panel.close + (size_t)pd * N, N, p.cfg.initial != 0);
        // single stock, initial=True: the state's shares are `[0] * stock_dim` (:415-422) while
        // asset_memory[0] (a0) counts num_stock_shares (:85-91, :364-370)
        if (p.cfg.single_ticker && p.cfg.initial) hf[0] = 0;
        const double b0 = initial_asset(cash, hf, p.panel.close + (size_t)pd * N, N, false);
        if (sel) {
            SF(FINENV_SF_CASH) = cash;
            SF(FINENV_SF_BEGIN_ASSET) = b0;     // sequential order: the first step's begin asset
#pragma unroll
            for (int i = 0; i < kNPad; ++i)
                if (i < N) HOLD(i) = hf[i];
            store_episode_start(p, E, e, a0, start);
            SI(FINENV_SI_DAY) = start;
            SI(FINENV_SI_PRICE_DAY) = pd;
            SF(FINENV_SF_TURBULENCE) = 0.0;
            SF(FINENV_SF_COST) = 0.0;
            SI(FINENV_SI_TRADES) = 0;
            if (mode == 0) {
                SI(FINENV_SI_EPISODE) = 0;
                SF(FINENV_SF_LAST_REWARD) = 0.0;
            } else {
                SI(FINENV_SI_EPISODE) += 1;
            }
        }
    }
    if (mode == 0 || p.obs == nullptr) return;
    lds[lane * kRow] = (float)cash;
#pragma unroll
    for (int i = 0; i < kNPad; ++i)
        if (i < N) lds[lane * kRow + 1 + i] = (float)hf[i];
    wave_sync();
    write_obs_rows(p.obs, p.panel.obs_tmpl, D, P, N, e0, nenv_w, pd, __ballot(sel), lds, lane);
}

