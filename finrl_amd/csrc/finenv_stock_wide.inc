// finenv_stock_wide.inc -- step kernel for a COMPILE-TIME ticker count NT in (64, 128]
// (NASDAQ-100: NT = 100, BASELINE configs[3]); included by finenv_stock_width.inc after
// finenv_stock_kernels.inc (shares its helpers and the aux kernel) and instantiated in namespace np128 alone.
//
// Same arithmetic as stock_step_kernel (env_stocktrading.py:220-357), different resource plan.
// The generic 128-wide kernel keeps the f32 action tile, 32-bit sorted keys and f32 observation rows
// in 67 KB of LDS -> two blocks per CU -> half the chip's SIMDs idle and two rounds of blocks at
// 65,536 envs (profiles/r02_head_n100_phase_timeline.txt).  This one fits 40.7 KB -> four blocks
// per CU, all 1024 blocks of a 65,536-env batch resident at once, one trader wave per SIMD:
//   * sorted keys are parked as 16-bit values (a * 128 + i fits int16 for |a| <= 255: larger hmax
//     goes to the generic kernel, and a scaled action beyond +-255 saturates there);
//   * the action tile never sits in LDS as a whole: the trader copies it through the (not yet
//     used) key region half a tile at a time -- coalesced 16-B loads, flat ds_write_b128, then
//     every lane reads ITS OWN 400-B row back with ds_read_b128 (rows 100 dwords apart: the 16
//     lanes of a b128 group cover all 64 banks) -- no per-element index arithmetic;
//   * holdings are [NT][65] (stride 65): the trade loops' per-lane dynamic ticker index stays
//     conflict-poor AND the observation writer can read them TRANSPOSED (lane = column) without a
//     second, row-major copy of the rows;
//   * the sorting network is Batcher's 128-input network pruned to the comparators below wire NT
//     (1104 instead of 1471 at NT = 100; absent inputs act as +inf parked on the top wires);
//   * the trader stages everything itself (holdings, price rows, tile), so the streamer depends on
//     the day index alone and writes from the first microsecond: the 52 MB of start-up reads
//     overlap with its stores (the step is HBM-bound: 370 MB per launch);
//   * ONE barrier, late: the
//     streamer copies the market-data chunks; the trader -- finished with its trades
//     ~7 us before the streamer has issued its last store -- writes the cash/holdings chunks of all
//     64 rows itself, ONE 16-byte-per-lane store per row (those four chunks are exactly 256 columns
//     at NT = 100; their market-data quads are loaded before the trade loops and wait in four
//     registers), THEN meets the streamer at the barrier (which also orders the streamer's read of the
//     day counters before their write-back); after it the two share the holdings write-back and the
//     trader writes the scalars.  It used to sit at a hand-off barrier until the streamer arrived
//     (37.5 -> 44.2 us in profiles/r02_n100_phase_timeline.txt), after which both waves needed 9 us
//     for 128 dword stores each.  Same-box A/B of the two forms: equal (profiles/r03_wide_attempts.md)
//     -- the launch is bound by the chip's store throughput, and the XCDs do not get equal shares of
//     it: blocks on XCC 1/3/5/7 finish ~10 us after those on XCC 0/2/4/6 in every run.
// Two things measured on the way (profiles/r02_wide_attempts.md) shape the code:
//   * straight-line code is NOT free: with every block resident and starting together, each 64-B
//     line of never-before-executed code costs an L2 round trip under full store load (~500
//     cycles = ~40 cycles per instruction); an all-in-registers variant (keys never parked, trade
//     loops unrolled over 100 ranks, 130 KB of code) ran the sort in 27 us and the buys in 55 us.
//     Everything after the sort is therefore a rolled loop over LDS-resident keys;
//   * a dependent global load under that store load costs ~2 us, so prices are staged once in LDS
//     (one shared row per block on lock-step days); per-lane action-row loads (64 lines per
//     instruction) took 13 us.

// native 4-float vector: HIP's float4 is a struct whose copies (register array -> LDS) reached the
// optimiser as memcpy and kept the whole action tile in scratch
typedef float wide_f4 __attribute__((ext_vector_type(4)));

template <int NT>
struct WideGeom {
    static constexpr int kHS = kWave + 1;                 // holdings row stride (dwords)
    static constexpr int kH = NT * kHS;                   // dwords: holdings [NT][65]
    static constexpr int kC = kHS;                        // dwords: f32 cash [64] = row NT of the image
    static constexpr int kPOff = (kH + kC + 1) & ~1;      // dword offset of the f64 price rows
    static constexpr int kP = 4 * NT;                     // dwords: current + next row (f64)
    static constexpr int kKOff = (kPOff + kP + 3) & ~3;   // dword offset of the key region (16-B aligned)
    static constexpr int kK = NT * kWave / 2;             // dwords: int16 keys [rank][64] == half an
                                                          // action tile (32 rows x NT f32)
    static constexpr int kDwords = kKOff + kK;
    static constexpr size_t kBytes = sizeof(float) * kDwords;
    static constexpr int kMaxHmax = (32767 - 127) / 128;  // 255: a * 128 + i must fit int16
};

// Batcher network of the 128-wide build pruned to wires < NT.
template <int NT>
__device__ __forceinline__ void sort_keys_pruned(int (&k)[NT])
{
#define CE(i, j) if constexpr ((j) < NT) ce(k[i], k[j]);
#include "sortnet128.inc"
#undef CE
}

// WIN: per-env episode windows (Params::win), as in stock_step_kernel
template <bool TURB, bool STATS, int NT, bool WIN = false>
__global__ void __launch_bounds__(kStepThreads, 2)
stock_step_wide_kernel(const Params p)
{
    static_assert(NT > 64 && NT <= 128 && NT % 4 == 0, "wide kernel: 64 < NT <= 128, NT % 4 == 0");
    using G = WideGeom<NT>;
    constexpr int kHS = G::kHS;
    extern __shared__ __attribute__((aligned(16))) float lds_all[];
    int *ldsh = reinterpret_cast<int *>(lds_all);                    // holdings [ticker][65]
    float *ldsc = lds_all + G::kH;                                   // f32 cash [env]
    double *ldsp = reinterpret_cast<double *>(lds_all + G::kPOff);   // price rows: cur [NT], next [NT]
    short *ldsk = reinterpret_cast<short *>(lds_all + G::kKOff);     // int16 sorted keys [rank][64]
    wide_f4 *ldst = reinterpret_cast<wide_f4 *>(lds_all + G::kKOff); // before that: half an action tile
    const int lane = threadIdx.x & (kWave - 1);
    // (readfirstlane: a SCALAR role makes the role split a real branch for the register allocator;
    //  as a per-lane value the streamer's 100 staging registers and the trader's action tile were
    //  live at the same time and the tile went to scratch)
    const int role = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // 0 trader, 1 streamer

    constexpr int N = NT;
    constexpr int kHoldSplit = NT / 2;                    // holdings [0, split) written back by the trader
    const int E = p.cfg.n_envs, D = p.D, T = p.cfg.n_days, P = p.obs_pitch;
    const int e0 = ((int)blockIdx.x + p.block_base) * kWave;
    if (e0 >= E) return;                                  // block-uniform
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;                 // clamped: tail lanes shadow env e0

    STAMP(0);
#ifdef FINENV_DIAG
    if (p.dbg != nullptr && lane == 0) p.dbg[((size_t)blockIdx.x * kStampRoles + role) * 16 + 14] = __builtin_amdgcn_s_memtime();
    // where this wave runs: XCC_ID (hwreg 20) in bits 0..7, HW_ID (hwreg 4: wave / simd / cu / sh / se) above
    if (p.dbg != nullptr && lane == 0)
        p.dbg[((size_t)blockIdx.x * kStampRoles + role) * 16 + 13] =
            (unsigned long long)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xff) |
            ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) << 8);
#endif
    // ---- trader: every global load it needs, issued before anything else: holdings (coalesced rows
    // of the state block), the two shared price rows (lane l loads tickers l, l + 64), then the
    // block's action tile [nenv_w][NT] f32, flat and coalesced (16 B per lane per load) -----------
    constexpr int kTileLoads = NT / 4;                    // float4 loads per lane = 64 * NT / 4 / 64
    constexpr int kHalves = (NT + kWave - 1) / kWave;
    const int act_n4 = nenv_w * (NT / 4);
    wide_f4 av[kTileLoads];
    int hv[NT];
    double pv[kHalves], pn[kHalves];
    if (role == 0) {
#pragma unroll
        for (int i = 0; i < NT; ++i) hv[i] = HOLD(i);
#pragma unroll
        for (int j = 0; j < kTileLoads; ++j) {
            const int idx4 = j * kWave + lane;
            av[j] = *reinterpret_cast<const wide_f4 *>(
                at(p.actions, (unsigned)(e0 * NT + 4 * (idx4 < act_n4 ? idx4 : 0))));
        }
    }
    // ---- both roles: which panel rows this step touches (needs only day / price_day) -----------
    int day = SI(FINENV_SI_DAY);
    int pd = SI(FINENV_SI_PRICE_DAY);
    const int last_day = WIN ? win_last_day(p.win, E, e, T) : T - 1;         // window end - 1
    const bool term = day >= last_day;                                        // :221
    const bool do_reset = term && p.auto_reset != 0;
    const int pd_cur = pd;                            // row held in the current observation
    const int pd_next = term ? pd : day + 1;          // row after the step, before any reset
    int reset_row = 0;                                // the window start (once per episode)
    if (WIN && !p.cfg.reset_quirk && __any(do_reset)) reset_row = win_start(p.win, e, T);
    const int row_obs = do_reset ? (p.cfg.reset_quirk ? pd : reset_row) : pd_next;
    const unsigned long long valid_mask = __ballot(valid);
    const unsigned long long term_mask = __ballot(term && valid);
    constexpr int kpatch = (2 * N) / kWave + 1;       // chunks holding cash/holdings columns
    const int pd_first = __builtin_amdgcn_readfirstlane(pd_cur);
    const bool uniform_pd = __all(pd_cur == pd_first);                        // same in both waves
    const int pn_first = __builtin_amdgcn_readfirstlane(pd_next);
    const bool uniform_next = __all(pd_next == pn_first);
    if (role == 0) {
#pragma unroll
        for (int half = 0; half < kHalves; ++half) {
            const int i = half * kWave + lane, ic = i < N ? i : 0;
            pv[half] = *at(p.panel.close, (unsigned)(pd_first * N + ic));
            pn[half] = *at(p.panel.close, (unsigned)(pn_first * N + ic));
        }
    }
    STAMP(1);

    // per-env values published in LDS for the observation writer: sel 0 = cash, 1 + i = holdings i
    // (the f32 cash row sits right behind the holdings: row NT of the same [.][kHS] word image)
    auto patch = [ldsh](int el, int sel) -> float {
        const int bits = ldsh[(sel == 0 ? NT : sel - 1) * kHS + el];
        return sel == 0 ? __int_as_float(bits) : (float)bits;
    };
    // head chunks (see head_plan / head_store): word index of a column in that image, transposed
    // reads (lane = column, stride kHS = 65: conflict-free)
    auto head_widx = [](int col) {
        const int hidx = col - 1 - NT;
        return col == 0 ? NT * kHS : ((hidx >= 0 && hidx < NT) ? hidx * kHS : -1);
    };
    auto head_val = [ldsh](int el, int w) -> float {
        const int bits = ldsh[w + el];
        return w == NT * kHS ? __int_as_float(bits) : (float)bits;
    };
    HeadPlan<kpatch> hp;
    const int ro_first = __builtin_amdgcn_readfirstlane(row_obs);
    // their template values: fetched by the trader during the trade phase (it has no stores in
    // flight then), parked in the key region once the keys are dead, read back after the barrier
    float *ldshead = lds_all + G::kKOff;

    if (role == 1) {
        // =========================== streamer ==================================================
        // part 1: nothing to stage -- the streamer needs the day index only and starts writing at
        // once (the start-up reads of the trader overlap with these stores: the step is HBM-bound);
        STAMP(2);
        STAMP(3);
        // part 2: market-data chunks of the observation rows
        // (one call site, two passes on episode-end steps: the writer is ~3 KB of code inlined)
        if (!DIAG(1)) {
#pragma nounroll
            for (int pass = (term_mask != 0ull && p.term_obs != nullptr) ? 0 : 1; pass < 2; ++pass)
                write_obs_rows(pass == 0 ? p.term_obs : p.obs, p.panel.obs_tmpl, D, pass == 0 ? D : P, N, e0, nenv_w,
                               pass == 0 ? pd_cur : row_obs, pass == 0 ? term_mask : valid_mask,
                               lds_all, lane, kpatch);
        }
        STAMP(4);
        // ONE barrier: (i) it orders this wave's read of the day counters (consumed long ago) before the
        // trader's write-back of them, which follows the same barrier; (ii) the trader, done with its trades
        // ~7 us earlier, has published its final holdings in LDS and issued its head-row stores by the time
        // it gets here: the upper part of the holdings write-back is done by this wave.
        lds_barrier();
        if (valid) {
#pragma unroll 10
            for (int i = kHoldSplit; i < N; ++i) HOLD(i) = ldsh[i * kHS + lane];
        }
        return;                                    // the trader writes every other per-env value itself
    }

    // =========================== trader wave only below =======================================
    double cash = SF(FINENV_SF_CASH);
    const double begin = SF(FINENV_SF_BEGIN_ASSET);
    double cost = SF(FINENV_SF_COST);
    int trades = SI(FINENV_SI_TRADES);
    double last_reward = SF(FINENV_SF_LAST_REWARD);
    double turb = 0.0, st_mean = 0.0, st_m2 = 0.0;
    bool first_step = false;                      // first step of this env's episode (STATS)
    if (TURB) turb = SF(FINENV_SF_TURBULENCE);
    if (STATS) {
        first_step = day == SI(FINENV_SI_START_DAY);
        st_mean = SF(FINENV_SF_RET_SUM);
        st_m2 = SF(FINENV_SF_RET_SUMSQ);
    }
    const bool turbulent = TURB && (turb >= p.cfg.turbulence_threshold);      // :308-310
    const int hmax = p.cfg.hmax;
    const float hmaxf = (float)hmax;
    double risk_next = 0.0;
    if (TURB) risk_next = *at(p.panel.risk, (unsigned)pd_next);

    // ---- holdings -> LDS [ticker][65]; shared price rows (sign bit of a close = the day's untradable
    // flag, :105/:174; the next row is only ever used as |close|) -------------------------------
#pragma unroll
    for (int i = 0; i < NT; ++i) ldsh[i * kHS + lane] = hv[i];
#pragma unroll
    for (int half = 0; half < kHalves; ++half) {
        const int i = half * kWave + lane;
        if (i < N) {
            ldsp[i] = pv[half];
            ldsp[NT + i] = fabs(pn[half]);
        }
    }
    // ---- action tile -> this lane's own row: two half tiles (32 envs x NT f32 = the key region's
    // size) copied flat into LDS and read back row-wise.  Row r starts at dword r * NT: for NT = 100
    // the 16 lanes of a ds_read_b128 group start 36 banks apart modulo 64 -- conflict-free.
    wide_f4 rowv[NT / 4];
    constexpr int kHalf4 = 32 * (NT / 4);                 // float4s per half tile
    // (two explicit passes: with the half index as a loop variable hipcc left av[] in scratch)
    auto copy_half = [&](auto half_c) {
        constexpr int half = decltype(half_c)::value;
#pragma unroll
        for (int j = 0; j < kTileLoads; ++j) {
            // float4 j*64 + lane of the tile belongs to this half iff it lies in [half, half+1) * kHalf4
            constexpr int lo = half * kHalf4, hi = lo + kHalf4;
            if (j * kWave + kWave <= lo || j * kWave >= hi) continue;        // static
            const int idx4 = j * kWave + lane;
            if (idx4 >= lo && idx4 < hi) ldst[idx4 - lo] = av[j];
        }
        wave_sync();
        if ((lane >> 5) == half) {
#pragma unroll
            for (int j = 0; j < NT / 4; ++j) rowv[j] = ldst[(lane & 31) * (NT / 4) + j];
        }
        wave_sync();
    };
    copy_half(std::integral_constant<int, 0>{});
    copy_half(std::integral_constant<int, 1>{});
    int keys[NT];
#pragma unroll
    for (int j = 0; j < NT / 4; ++j) {
        const float c[4] = {rowv[j].x, rowv[j].y, rowv[j].z, rowv[j].w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = 4 * j + u;
            const float x = c[u] * hmaxf;                                     // f32 mul, :304
            int a = (int)x;                                                   // trunc, :305
            // saturates at what the int16 park below holds (include/finenv.h, "Action domain"): an
            // action beyond it stays a trade of its own sign instead of wrapping into the other one
            a = max(-G::kMaxHmax, min(G::kMaxHmax, a));
            a = turbulent ? -hmax : a;
            a = term ? 0 : a;                                                 // no trading
            keys[i] = a * kNPad + i;      // unique; order == stable argsort(actions), :317
        }
    }
    STAMP(2);
    wave_sync();                                   // holdings / price rows visible to every lane
    STAMP(3);
    if (!DIAG(4)) sort_keys_pruned<NT>(keys);
    STAMP(5);

    // ---- park the sorted keys as int16 [rank][lane] (the tile is dead) ---------------------------
    wave_sync();
#pragma unroll
    for (int r = 0; r < NT; ++r) ldsk[r * kWave + lane] = (short)keys[r];
    const short *kcol = ldsk + lane;               // this env's sorted keys, stride kWave
    int *hcol = ldsh + lane;                       // this env's holdings by ticker, stride kHS
    // signed close of ticker idx on this env's current day (sign bit = untradable flag)
    auto price_signed = [&](int idx) -> double {
        if (uniform_pd) return ldsp[idx];
        return *at(p.panel.close, (unsigned)(pd_cur * N + idx));
    };

    // ---- begin_total_asset (:311-314) is carried over from the previous step's end asset (see
    // FINENV_SF_BEGIN_ASSET in include/finenv.h): 100 LDS reads + fp64 multiply-adds less on the
    // trader's path (6.7 us in profiles/r02_wide_v3_phase_timeline.txt)
    double s = 0.0;
    wave_sync();
    STAMP(4);
    float head_tt[kpatch] = {};                    // in flight during the trade loops
    typedef wide_f4 wide_f4u __attribute__((aligned(4)));
    // quad form (no hand-off): lane l holds columns 4l .. 4l+3 of the 64 * kpatch head columns
    constexpr bool kQuadHead = kpatch == 4;
    wide_f4 head_q = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kQuadHead && D >= kpatch * kWave)
        head_q = *reinterpret_cast<const wide_f4u *>(
            reinterpret_cast<const char *>(p.panel.obs_tmpl) + (size_t)((unsigned)(ro_first * D + 4 * lane) * 4u));
    else
        head_fetch(head_tt, p.panel.obs_tmpl, D, ro_first, lane, kpatch);

    const double c_s = p.cfg.sell_cost_pct, c_b = p.cfg.buy_cost_pct;
    const double one_m_cs = 1 - c_s, one_p_cb = 1 + c_b;

    if (uniform_pd) {
        // ---- lock-step days: rank-ordered register chunks.  Keys of a chunk are read back by rank
        // (static stride), their (price, holdings) gathered with the whole chunk's LDS loads in
        // flight, the chunk then applied straight-line; ROLLED over chunks (code size, see top).
        // sells: most negative first (:317-324, _sell_stock :102-169).  Share counts do not depend
        // on cash; cash / cost are summed in rank order; ranks that sell nothing add +0.0.
        if (!DIAG(2)) {
            constexpr int kChS = NT % 20 == 0 ? 20 : 16;           // NT = 100: five full chunks
            static_assert(NT % kChS == 0, "sell chunks must tile the ranks");
            int n_sold = 0;
#pragma nounroll
            for (int c = 0; c < NT; c += kChS) {
                if (!__any(kcol[c * kWave] < 0)) break;            // sorted ascending
                int kk[kChS], hS[kChS];
                double pS[kChS];
#pragma unroll
                for (int r = 0; r < kChS; ++r) kk[r] = kcol[(c + r) * kWave];
#pragma unroll
                for (int r = 0; r < kChS; ++r) {
                    const int idx = kk[r] & (kNPad - 1);
                    pS[r] = ldsp[idx];
                    hS[r] = hcol[idx * kHS];
                }
#pragma unroll
                for (int r = 0; r < kChS; ++r) {
                    const int key = kk[r];
                    const int h = hS[r];
                    const int phi = __double2hiint(pS[r]);     // sign bit = untradable flag
                    // all-ones iff key < 0 and h > 0 and (turbulent ? price != 0 : tradable)
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
                    // (q == 0 rewrites the same value; a ticker belongs to exactly one rank)
                    hcol[(key & (kNPad - 1)) * kHS] = h - q;                      // :123
                }
            }
            trades += n_sold;
        }
        STAMP(6);
        // buys: largest first (:319, :328-330, _buy_stock :171-213).  Serial through cash:
        // q = min(a, cash // unit), cash -= p*q*(1+c_b); `cash // unit` is floor(cash * (1/unit))
        // clamped to a, made exact by the sign of one FMA remainder.
        if (!DIAG(2)) {
            constexpr int kChB = NT % 10 == 0 ? 10 : 8;
            static_assert(NT % kChB == 0, "buy chunks must tile the ranks");
            // Software pipeline over chunks: while chunk c is applied, the keys of chunk c+1 are in
            // flight; its prices, unit costs and reciprocals are prepared right after the chain, so
            // the next iteration starts on the cash chain at once.
            int kk[kChB];
            double pB[kChB], uB[kChB], xB[kChB];
#pragma unroll
            for (int j = 0; j < kChB; ++j) kk[j] = kcol[(NT - 1 - j) * kWave];
#pragma unroll
            for (int j = 0; j < kChB; ++j) {
                pB[j] = ldsp[kk[j] & (kNPad - 1)];
                uB[j] = pB[j] * one_p_cb;                                         // :179
                xB[j] = refined_rcp(uB[j]);
            }
#pragma nounroll
            for (int hi = NT - 1; hi >= 0; hi -= kChB) {
                if (!__any(kk[0] >= kNPad)) break;                 // sorted: no buys (a >= 1) below
                int kn[kChB];
#pragma unroll
                for (int j = 0; j < kChB; ++j) kn[j] = kcol[max(hi - kChB - j, 0) * kWave];
#pragma unroll
                for (int j = 0; j < kChB; ++j) {
                    // (no early exit inside a chunk: ranks without a buy are exact no-ops)
                    const int key0 = kk[j];
                    const int a0 = key0 >> kLog2NPad;
                    const double ad = (double)a0;
                    const bool ok = key0 >= kNPad && !turbulent && uB[j] > 0.0;   // u <= 0: flagged / no price
                    double q0;                                                    // :178-184
                    {
                        const double f = floor(cash * xB[j]);
                        asm("v_min_f64 %0, %1, %2" : "=v"(q0) : "v"(f), "v"(ad));
                    }
                    const double rem = fma(-q0, uB[j], cash);
                    int qi = (int)q0;
                    qi += ((rem >= uB[j]) & (qi < a0)) ? 1 : 0;
                    qi -= (rem < 0.0) ? 1 : 0;
                    qi = ok ? qi : 0;                          // q = 0 leaves cash / cost bit-identical
                    const double amt = pB[j] * (double)qi;
                    cash = cash - amt * one_p_cb;                                 // :185-190
                    cost = cost + amt * c_b;                                      // :194-196
                    trades += ok ? 1 : 0;                                         // :197
                    __hip_atomic_fetch_add(&hcol[(key0 & (kNPad - 1)) * kHS], qi, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WAVEFRONT);          // :192
                }
#pragma unroll
                for (int j = 0; j < kChB; ++j) {
                    kk[j] = (hi - kChB >= 0) ? kn[j] : 0;          // past the last chunk: no buys
                    pB[j] = ldsp[kk[j] & (kNPad - 1)];
                    uB[j] = pB[j] * one_p_cb;                                     // :179
                    xB[j] = refined_rcp(uB[j]);
                }
            }
        }
    } else {
        // ---- envs of this block sit on different days (random starts): prices gathered per rank
        // from the panel; plain rolled loops, two-deep software pipeline (the generic kernel's form)
        if (!DIAG(2)) {
            int key0 = kcol[0];
            int key1 = kcol[1 * kWave];
            int h0 = hcol[(key0 & (kNPad - 1)) * kHS];
            double q0p = price_signed(key0 & (kNPad - 1));
            int n_sold = 0;
#pragma unroll 2
            for (int r = 0; r < NT; ++r) {
                if (!__any(key0 < 0)) break;               // sorted: no sells beyond this rank
                const int key2 = kcol[min(r + 2, NT - 1) * kWave];
                const int i1 = key1 & (kNPad - 1);
                const int h1 = hcol[i1 * kHS];
                const double p1 = price_signed(i1);
                const int idx = key0 & (kNPad - 1);
                const int a = key0 >> kLog2NPad;
                const bool ok = key0 < 0 && h0 > 0 &&
                                (turbulent ? (fabs(q0p) > 0.0) : !__builtin_signbit(q0p));
                const int q = ok ? (turbulent ? h0 : min(-a, h0)) : 0;
                hcol[idx * kHS] = h0 - q;                                         // :123
                n_sold += ok ? 1 : 0;                                             // :129
                const double amt = fabs(q0p) * (double)q;
                cash = cash + amt * one_m_cs;                                     // :115-121
                cost = cost + amt * c_s;                                          // :124-128
                key0 = key1; key1 = key2; h0 = h1; q0p = p1;
            }
            trades += n_sold;
        }
        STAMP(6);
        if (!DIAG(2)) {
            int key0 = kcol[(NT - 1) * kWave];
            int key1 = kcol[(NT - 2) * kWave];
            double p0 = price_signed(key0 & (kNPad - 1));
            double u0 = p0 * one_p_cb;                                            // :179
            double x0 = refined_rcp(u0);
#pragma unroll 2
            for (int r = NT - 1; r >= 0; --r) {
                if (!__any(key0 >= kNPad)) break;          // sorted: no buys (a >= 1) below this rank
                const int key2 = kcol[max(r - 2, 0) * kWave];
                const double p1 = price_signed(key1 & (kNPad - 1));
                const double u1 = p1 * one_p_cb;
                const double x1 = refined_rcp(u1);
                const int idx = key0 & (kNPad - 1);
                const double ad = (double)(key0 >> kLog2NPad);
                const bool ok = key0 >= kNPad && !turbulent && u0 > 0.0;
                const double q0 = fmin(floor(cash * x0), ad);                     // :178-184
                const double rem = fma(-q0, u0, cash);
                const double adj = ((rem < 0.0) ? -1.0 : 0.0) + ((rem >= u0 && q0 < ad) ? 1.0 : 0.0);
                const double qd = ok ? q0 + adj : 0.0;     // q = 0 leaves cash / cost bit-identical
                const double amt = p0 * qd;
                cash = cash - amt * one_p_cb;                                     // :185-190
                cost = cost + amt * c_b;                                          // :194-196
                trades += ok ? 1 : 0;                                             // :197
                __hip_atomic_fetch_add(&hcol[idx * kHS], (int)qd, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WAVEFRONT);              // :192
                key0 = key1; key1 = key2; p0 = p1; u0 = u1; x0 = x1;
            }
        }
    }
    STAMP(7);

    // ---- day += 1, new row, end_total_asset (:335-347) -----------------------------------------
    if (!term) {
        day += 1;
        pd = day;
        if (TURB) turb = risk_next;
    }
    wave_sync();
    s = 0.0;
    if (uniform_next) {                      // next row staged (as |close|) by the streamer
#pragma unroll 10
        for (int i = 0; i < N; ++i) s = s + ldsp[NT + i] * (double)hcol[i * kHS];
    } else {
        const unsigned nb = (unsigned)(pd_next * N);
#pragma unroll 10
        for (int i = 0; i < N; ++i)
            s = s + fabs(*at(p.panel.close, nb + (unsigned)i)) * (double)hcol[i * kHS];
    }
    ldsc[lane] = (float)cash;
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
            *at(p.realised, (unsigned)(e * N + i)) = hcol[i * kHS] - HOLD(i);
    }
    STAMP(9);
    wave_sync();

    // ---- terminal observation; auto-reset (once per episode, wave-uniform) ---------------------
    int episode_inc = 0;
    if (term_mask != 0ull) {
        // last-episode block: before the auto-reset below rewrites the state.  At `term` the end
        // asset equals the carried begin asset (no trade, same row); the STATS kernels keep `end`
        // live for the Sharpe sums anyway, the others hand over end_carry (live until write-back).
        if (p.last != nullptr && term && valid) latch_last_episode(p, p.last, E, e, STATS ? end : end_carry);
        if (p.term_obs != nullptr)
            write_obs_rows_fn(p.term_obs, p.panel.obs_tmpl, D, D, N, e0, nenv_w, pd_cur, term_mask,
                              patch, lane, 0, kpatch);       // (once per episode: compact generic form)
        if (p.auto_reset) {                  // reset(), :359-393
            wave_sync();
            if (term) {
                pd = row_obs;
                cash = SF(FINENV_SF_CASH0);
                for (int i = 0; i < N; ++i) hcol[i * kHS] = SH0(i);
                ldsc[lane] = (float)cash;
                const double a0 = initial_asset_lds(cash, hcol, p.panel.close, (unsigned)(pd * N),
                                                    N, p.cfg.initial != 0, kHS);
                end_carry = initial_asset_lds(cash, hcol, p.panel.close, (unsigned)(pd * N), N, false,
                                              kHS);
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

    const bool quad_rows = kQuadHead && D >= kpatch * kWave &&
                           __all(!valid || row_obs == ro_first);         // every env shows the same row
    wave_sync();                                   // this wave's own LDS image (cash, holdings) is final
    if (!quad_rows) {
        head_park(ldshead, head_tt, lane);         // (head_tt was fetched iff the quad form is off)
        wave_sync();
        head_plan(hp, ldshead, D, row_obs, ro_first, valid_mask, lane, kpatch, head_widx);
    }
    // ---- the cash / holdings chunks of all 64 rows, one 16-byte store per row.  Column
    // c = 4 * lane + u: cash (c == 0), holdings c - 1 - NT, else the market-data value loaded above.
    if (quad_rows && !DIAG(1)) {
        int w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = head_widx(4 * lane + u);
        char *const hb = reinterpret_cast<char *>(p.obs + (size_t)e0 * P);
        constexpr int kB = 8;                     // rows per batch: their LDS reads before their stores
        for (int g = 0; g < nenv_w; g += kB) {
            float pv4[kB][4];
#pragma unroll
            for (int j = 0; j < kB; ++j)
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    pv4[j][u] = head_val(min(g + j, kWave - 1), w[u] >= 0 ? w[u] : 0);
#pragma unroll
            for (int j = 0; j < kB; ++j) {
                const int el = g + j;
                if (el >= nenv_w) continue;
                wide_f4 v;
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = w[u] >= 0 ? pv4[j][u] : head_q[u];
                *reinterpret_cast<wide_f4u *>(hb + (size_t)((unsigned)(el * P + 4 * lane) * 4u)) = v;
            }
        }
    }
    // ---- the observation chunks holding cash / holdings (:342 / :453-478) when the quad form did not
    // write them (rows on different panel rows, fewer than 256 columns) -----------------------------
    if (!DIAG(1) && !quad_rows) {
        if (hp.uniform)
            head_store(hp, p.obs, D, P, e0, nenv_w, valid_mask, lane, 0, kWave, head_val);
        else
            write_obs_rows_fn(p.obs, p.panel.obs_tmpl, D, P, N, e0, nenv_w, row_obs, valid_mask, patch,
                              lane, 0, kpatch, 0, kWave);
    }
    // ---- hand-off barrier (see the streamer): this wave's head-row stores are in flight; everything that
    // overwrites what the streamer read at its start comes after it --------------------------------------
    lds_barrier();
    // ---- state write-back -----------------------------------------------------------------------------
    if (valid) store_trader<TURB>(p, E, e, cash, end_carry, cost, trades, day, pd, last_reward, turb, episode_inc);
    // running sums for the terminal Sharpe (:243-251): the rule of store_sharpe_sums, finenv_stock_common.h; this
    // kernel keeps its copy (the call changed the code of its four STATS instantiations, profiles/stock_one_rule.md)
    if (STATS && !term) {
        double st_prev = begin;
        if (__any(first_step)) {
            const double a0 = SF(FINENV_SF_ASSET0);
            st_prev = first_step ? a0 : begin;
        }
        const double ret = end / st_prev - 1.0;
        if (valid) {
            SF(FINENV_SF_RET_SUM) = st_mean + ret;
            SF(FINENV_SF_RET_SUMSQ) = st_m2 + ret * ret;
        }
    }
    if (valid) {
#pragma unroll 10
        for (int i = 0; i < kHoldSplit; ++i) HOLD(i) = hcol[i * kHS];
    }
    STAMP(10);
    STAMP(11);
    stamp_wave_end(p, lane, role);
}
