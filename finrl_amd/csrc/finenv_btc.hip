// finenv_btc.hip -- MI355X (gfx950) kernel + C ABI for the batched single-asset BitcoinEnv.
//
// Replaces finrl/meta/env_cryptocurrency_trading/env_btc_ccxt.py step() :81-129 and reset() :53-79
// for E independent envs per launch.  NOT the N = 1 case of the CryptoEnv kernel: this env may go
// short (down to -0.5 * total_asset / price), buys fractional amounts capped by account / price
// with the fee outside the cap, adds the discounted return to the terminal reward instead of
// replacing it, and shows every price column in its observation (the contract is in include/finenv.h).
//
// lane = env, one wave per 64 envs, independent waves (no block barriers).  77 + 4 * D algorithmic
// bytes per env-step (D = P + 9 floats of observation): the step is latency-bound up to a few
// hundred thousand envs, so what counts is the number of DEPENDENT global round trips.  Two:
//   1. action, the four f64 state fields, day, stocks tag and (WIN) the window end -- all coalesced,
//      none depends on another;
//   2. price0[day], price0[day + 1] and the ready-made middle of the observation row of day + 1.
// Every load is issued before the first store (a load behind stores waits for their
// acknowledgement, DESIGN.md 4b rule (i)); the two exceptions run once per episode: the window
// start, read only in a step in which an env of the wave resets, and the terminal-observation rows.
// The wave's 64 observation rows are one contiguous 256 * D-byte run of the output: the per-env
// columns (account, stocks) and the template row(s) are parked in LDS and every lane stores 16
// bytes of the run at a time.  A batch in lock step parks ONE template row per wave (one coalesced
// load); envs of a wave on different days each park their own row.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "finenv.h"
#include "finenv_dev.h"
#include "finenv_host.h"

namespace {

typedef float wide4 __attribute__((ext_vector_type(4)));
constexpr int kWave = 64;
constexpr int kTmplChunks = 4;                  // 64-column chunks of the lock-step template row: M <= 256
constexpr int kMaxD = FINENV_BTC_MAX_PRICE_COLS + 9;   // 254: one wave's LDS (below) fits the 64 KB of a block
// LDS per wave (dwords): [64][D] the template part of the wave's observation rows (lock step: the
// one common row at its start), then [64][2] the per-env columns (account, stocks).  Both 16-byte
// aligned for every D.
__host__ __device__ constexpr int lds_per_wave(int D) { return kWave * D + 2 * kWave; }
__host__ __device__ constexpr int waves_per_block(int D) { return D <= 62 ? 4 : (D <= 126 ? 2 : 1); }

struct BtParams {
    finenv_btc_config cfg;
    finenv_btc_panel panel;
    finenv_btc_state st;
    const float *actions;
    float *obs;
    float *reward;
    uint8_t *done;
    float *term_obs;
    const uint8_t *mask;
    int32_t auto_reset;
    int32_t D;
    uint32_t magicD;              // ceil(2^32 / D): row of a flat index into the wave's [64][D] block
    const int32_t *win;           // finenv_btc_set_windows (the WIN instantiations; NULL otherwise)
};

#define BF(fld) (*at(p.st.f64, (unsigned)(fld) * (unsigned)E + (unsigned)e))
#define BI(fld) (*at(p.st.i32, (unsigned)(fld) * (unsigned)E + (unsigned)e))

// `stocks +/- q` as NumPy evaluates it for the scalar types behind the tags (:90, :95): the result
// has the wider of the two types (a Python float is weak: it takes the other's), and while that is
// float32 the operation itself is a float32 one -- a real one, not a rounded double result.
__device__ __forceinline__ double stocks_add(double s, int s_tag, double q, int q_tag, bool minus)
{
    const float s32 = (float)s, q32 = (float)q;               // (exact while the result tag is F32)
    const float r32 = minus ? s32 - q32 : s32 + q32;
    const double r64 = minus ? s - q : s + q;
    return max(s_tag, q_tag) == FINENV_NT_F32 ? (double)r32 : r64;
}

// The wave's observation rows -> dst[e0 * D ..]: flat float f of the run is row r = f / D, column
// c = f % D: account (c == 0) and stocks (c == D - 1) of env r from `heads`, else the template value
// img[r * rs + c - 1] (rs = 0: the wave's common row, rs = D: a row per env).  Full waves whose rows
// are all written and whose destination is 16-byte aligned store 16 bytes per lane; tail waves,
// masked resets and destinations such as slice t of a [n][E][D] tensor with E * D odd go by dwords.
__device__ __forceinline__ void bt_write_rows(float *__restrict__ dst, const BtParams &p, int e0,
                                              int nenv_w, unsigned long long row_mask,
                                              const float *img, int rs, const float *heads, int lane)
{
    const int D = p.D;
    const unsigned magicD = p.magicD;
    float *const base = dst + (size_t)e0 * (size_t)D;
    auto val = [&](int f) {
        const int r = (int)__umulhi((unsigned)f, magicD);
        const int c = f - r * D;
        return c == 0 ? heads[2 * r] : (c == D - 1 ? heads[2 * r + 1] : img[r * rs + c - 1]);
    };
    if (nenv_w == kWave && row_mask == ~0ull && ((uintptr_t)base & 15) == 0) {
        const int n4 = kWave * D / 4;
        wide4 *const dst4 = reinterpret_cast<wide4 *>(base);
#pragma unroll 2
        for (int j = lane; j < n4; j += kWave) {
            wide4 v;
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = val(4 * j + u);
            dst4[j] = v;
        }
    } else {
        const int total = nenv_w * D;
#pragma unroll 4
        for (int f = lane; f < total; f += kWave) {
            const int r = (int)__umulhi((unsigned)f, magicD);
            const float v = val(f);
            if ((row_mask >> r) & 1ull) *at(base, (unsigned)f) = v;
        }
    }
}

// park the template row `trow` of every lane's env in img[lane * D ..] (M = D - 2 values per lane,
// eight loads in flight at a time)
__device__ __forceinline__ void bt_park_own_rows(float *img, const BtParams &p, int trow, int lane)
{
    const int D = p.D, M = D - 2;
    const unsigned tb = (unsigned)(trow * M);
    for (int c0 = 0; c0 < M; c0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = *at(p.panel.obs_tmpl, tb + (unsigned)min(c0 + u, M - 1));
#pragma unroll
        for (int u = 0; u < 8; ++u) pin(v[u]);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (c0 + u < M) img[lane * D + c0 + u] = v[u];
    }
}

// WIN: per-env episode windows (finenv_btc_set_windows), int32 win[2][E]: env e runs panel rows
// [win[0][e], win[1][e]).  The end is loaded in round trip 1 of every step, the start only when an
// env of the wave resets; both are clamped into the panel (finenv_dev.h).
template <bool RESET_ONLY, bool WIN>
__global__ void __launch_bounds__(256) btc_kernel(const BtParams p)
{
    extern __shared__ __attribute__((aligned(16))) float lds_all[];   // [waves][lds_per_wave(D)]
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int E = p.cfg.n_envs, T = p.cfg.n_rows, D = p.D, M = D - 2;
    float *img = lds_all + wv * lds_per_wave(D);
    float *heads = img + kWave * D;
    const int e0 = (int)(blockIdx.x * (blockDim.x >> 6) + wv) * kWave;
    if (e0 >= E) return;
    const int nenv_w = min(kWave, E - e0);
    const bool valid = lane < nenv_w;
    const int e = valid ? e0 + lane : e0;

    if (RESET_ONLY) {                                       // reset(), :53-79
        const bool sel = valid && (p.mask == nullptr || p.mask[e] != 0);
        const int row = WIN ? win_start(p.win, e, T) : 0;
        const double price = *at(p.panel.price0, (unsigned)row);
        if (p.obs != nullptr) bt_park_own_rows(img, p, row, lane);
        const double account = p.cfg.initial_account;
        const double stocks = 0.0;
        if (sel) {                                          // (gamma_return, episode_return: untouched)
            BI(FINENV_BI_DAY) = row;
            BI(FINENV_BI_STOCKS_TAG) = FINENV_NT_PY;
            BF(FINENV_BF_ACCOUNT) = account;
            BF(FINENV_BF_STOCKS) = stocks;
            BF(FINENV_BF_TOTAL_ASSET) = account + price * stocks;                 // :60
        }
        if (p.obs == nullptr) return;
        heads[2 * lane] = (float)(account * 0x1p-18);
        heads[2 * lane + 1] = (float)(stocks * 0x1p-4);
        wave_sync();
        bt_write_rows(p.obs, p, e0, nenv_w, __ballot(sel), img, D, heads, lane);
        return;
    }

    // ---- round trip 1: nothing here depends on anything else; the day first (loads return in
    // order: it is the one value round trip 2 waits for) -------------------------------------------
    const int day_raw = BI(FINENV_BI_DAY);
    int w_last = T - 1;                                     // the terminal row: rows - 1, :101
    if (WIN) w_last = win_last_day(p.win, E, e, T);
    int tag = BI(FINENV_BI_STOCKS_TAG);
    const float x = *at(p.actions, (unsigned)e);                                  // :82
    double account = BF(FINENV_BF_ACCOUNT);
    double stocks = BF(FINENV_BF_STOCKS);
    double total = BF(FINENV_BF_TOTAL_ASSET);
    double gamma_ret = BF(FINENV_BF_GAMMA_RETURN);

    const int day = min(max(day_raw, 0), T - 1);            // (a panel row, whatever the state holds)
    // an env already on its terminal row (stepped again after done without a reset: the reference
    // raises IndexError) makes no trade, keeps its state and reports reward 0, done 1
    const bool past = day >= w_last;
    const int t_next = past ? day : day + 1;                                      // :98
    const bool done = past || t_next == w_last;                                   // :101
    const bool restart = done && p.auto_reset != 0;
    int t_show = t_next;                                    // the row of the observation this step returns
    if (p.auto_reset && __any(done && valid)) {
        const int s = WIN ? win_start(p.win, e, T) : 0;
        if (done) t_show = s;
    }

    // ---- round trip 2: the two prices of the trade and the revaluation, the template row(s) ------
    const double p0 = *at(p.panel.price0, (unsigned)day);                         // adj, :84
    const double p1 = *at(p.panel.price0, (unsigned)t_next);                      // :120
    const double ps = *at(p.panel.price0, (unsigned)t_show);                      // a restart's :60
    const int t_first = __builtin_amdgcn_readfirstlane(t_show);
    const bool uniform = __all(t_show == t_first) && M <= kTmplChunks * kWave;
    if (uniform) {
        float tt[kTmplChunks];
        const unsigned tb = (unsigned)(t_first * M);
#pragma unroll
        for (int k = 0; k < kTmplChunks; ++k)
            tt[k] = *at(p.panel.obs_tmpl, tb + (unsigned)min(k * kWave + lane, M - 1));
#pragma unroll
        for (int k = 0; k < kTmplChunks; ++k) pin(tt[k]);
#pragma unroll
        for (int k = 0; k < kTmplChunks; ++k)
            if (k * kWave + lane < M) img[k * kWave + lane] = tt[k];
    } else {
        bt_park_own_rows(img, p, t_show, lane);
    }

    // ---- the trade (:85-95), each operation rounded on its own, in the reference's order --------
    const double fee = p.cfg.transaction_fee_percent;
    if (!past && x < 0.0f) {
        const float want = -x;                                                    // -1 * a: float32
        const double cap = (0.5 * total) / p0 + stocks;                           // float64, :87
        const bool capped = cap < (double)want;             // min(): ties keep the first
        double q = capped ? cap : (double)want;
        const int q_tag = capped ? FINENV_NT_F64 : FINENV_NT_F32;
        if (q > 0.0) {                                      // max(0, q) keeps q
            account = account + (p0 * q) * (1 - fee);                             // :89
            stocks = stocks_add(stocks, tag, q, q_tag, true);                     // :90
            tag = max(tag, q_tag);
        } else {                                            // the int 0: stocks and its type stay
            q = 0.0;
            account = account + (p0 * q) * (1 - fee);
        }
    } else if (!past && x > 0.0f) {
        const double mx = account / p0;                                           // :92
        const bool capped = mx < (double)x;                                       // :93
        const double q = capped ? mx : (double)x;           // (no clamp: negative with the account)
        const int q_tag = capped ? FINENV_NT_F64 : FINENV_NT_F32;
        account = account - (p0 * q) * (1 + fee);                                 // :94
        stocks = stocks_add(stocks, tag, q, q_tag, false);                        // :95
        tag = max(tag, q_tag);
    }
    double reward = 0.0;
    double episode_ret = 0.0;
    if (!past) {
        const double next = account + p1 * stocks;                                // :120
        reward = (next - total) * 0x1p-16;                                        // :121
        total = next;
        gamma_ret = gamma_ret * p.cfg.gamma + reward;                             // :124
        if (done) {
            reward = reward + gamma_ret;                                          // :126
            gamma_ret = 0.0;
            episode_ret = next / p.cfg.initial_account;                           // :128
        }
    }

    // ---- terminal observations, once per episode: the row the reference's last step() returns,
    // before an auto-reset replaces it; each done env writes its own row -----------------------
    if (p.term_obs != nullptr && done && valid) {
        float *const tr = p.term_obs + (size_t)e * (size_t)D;
        const unsigned tb = (unsigned)(t_next * M);
        for (int c0 = 0; c0 < M; c0 += 8) {                 // (eight loads in flight, then their stores)
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *at(p.panel.obs_tmpl, tb + (unsigned)min(c0 + u, M - 1));
#pragma unroll
            for (int u = 0; u < 8; ++u) pin(v[u]);
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (c0 + u < M) tr[1 + c0 + u] = v[u];
        }
        tr[0] = (float)(account * 0x1p-18);
        tr[D - 1] = (float)(stocks * 0x1p-4);
    }

    // ---- outputs and state ----------------------------------------------------------------------
    if (valid) {
        *at(p.reward, (unsigned)e) = (float)reward;
        *at(p.done, (unsigned)e) = done ? 1 : 0;
        BF(FINENV_BF_LAST_REWARD) = reward;
        BF(FINENV_BF_GAMMA_RETURN) = gamma_ret;
        if (done && !past) BF(FINENV_BF_EPISODE_RETURN) = episode_ret;
    }
    if (restart) {                                          // reset(), :53-60
        account = p.cfg.initial_account;
        stocks = 0.0;
        tag = FINENV_NT_PY;
        total = account + ps * stocks;
    }
    heads[2 * lane] = (float)(account * 0x1p-18);                                 // :113
    heads[2 * lane + 1] = (float)(stocks * 0x1p-4);                               // :116
    if (valid) {
        BF(FINENV_BF_ACCOUNT) = account;
        BF(FINENV_BF_STOCKS) = stocks;
        BF(FINENV_BF_TOTAL_ASSET) = total;
        BI(FINENV_BI_DAY) = t_show;
        BI(FINENV_BI_STOCKS_TAG) = tag;
    }
    wave_sync();
    bt_write_rows(p.obs, p, e0, nenv_w, __ballot(valid), img, uniform ? 0 : D, heads, lane);
}

}  // namespace

struct finenv_btc : finenv_host::Handle {
    finenv_btc_config cfg;
    finenv_btc_panel panel;
    finenv_btc_state st;
    uint32_t magicD;
    int32_t *win;                 // finenv_btc_set_windows
};

namespace {
BtParams bt_params(const finenv_btc *h)
{
    BtParams p;
    memset(&p, 0, sizeof(p));
    p.cfg = h->cfg;
    p.panel = h->panel;
    p.st = h->st;
    p.D = h->D;
    p.magicD = h->magicD;
    p.win = h->win;
    return p;
}

template <bool RESET_ONLY>
void bt_launch(const BtParams &p, hipStream_t stream)
{
    const int waves = (p.cfg.n_envs + kWave - 1) / kWave;
    const int wpb = waves_per_block(p.D);
    const dim3 grid((unsigned)((waves + wpb - 1) / wpb)), block((unsigned)(kWave * wpb));
    const size_t lds = sizeof(float) * (size_t)lds_per_wave(p.D) * (size_t)wpb;
    if (p.win != nullptr)                                   // a window block is attached
        hipLaunchKernelGGL((btc_kernel<RESET_ONLY, true>), grid, block, lds, stream, p);
    else
        hipLaunchKernelGGL((btc_kernel<RESET_ONLY, false>), grid, block, lds, stream, p);
}
}  // namespace

extern "C" {

int finenv_btc_create(const finenv_btc_config *cfg, finenv_btc **out)
{
    if (!cfg || !out) return FINENV_ERR_INVALID;
    *out = nullptr;
    if (cfg->n_envs < 1 || cfg->n_price_cols < 1 || cfg->n_tech_cols < 7 || cfg->n_rows < 2)
        return FINENV_ERR_INVALID;
    const long long E = cfg->n_envs, P = cfg->n_price_cols, T = cfg->n_rows;
    const long long D = P + 9, lim = (1ll << 32) - 1;
    if (D > kMaxD || E * 8 * FINENV_BTC_F64_FIELDS > lim || E * D * 4 > lim || T * 8 > lim ||
        T * (D - 2) * 4 > lim)
        return FINENV_ERR_INVALID;
    finenv_btc *h = finenv_host::new_handle<finenv_btc>(cfg, D);
    if (!h) return FINENV_ERR_NOMEM;
    h->magicD = finenv_host::magic_for(D);
    *out = h;
    return FINENV_OK;
}

void finenv_btc_destroy(finenv_btc *h) { delete h; }
const char *finenv_btc_last_error(const finenv_btc *h) { return finenv_host::last_error(h); }
int finenv_btc_obs_dim(const finenv_btc *h) { return finenv_host::obs_dim(h); }

int finenv_btc_bind(finenv_btc *h, const finenv_btc_panel *panel, const finenv_btc_state *st)
{
    if (!h || !panel || !st) return FINENV_ERR_INVALID;
    if (!panel->price0 || !panel->obs_tmpl || !st->f64 || !st->i32)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "bind: null pointer");
    return finenv_host::bind(h, panel, st);
}

int finenv_btc_set_windows(finenv_btc *h, int32_t *win)
{
    if (!h) return FINENV_ERR_INVALID;
    h->win = win;
    return FINENV_OK;
}

int finenv_btc_reset(finenv_btc *h, const uint8_t *mask, float *obs_out, void *stream)
{
    if (const int rc = finenv_host::ready(h, "reset")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    BtParams p = bt_params(h);
    p.mask = mask;
    p.obs = obs_out;
    bt_launch<true>(p, (hipStream_t)stream);
    return finenv_host::check_launch(h, "btc_reset");
}

int finenv_btc_step(finenv_btc *h, const float *actions, float *obs, float *reward, uint8_t *done,
                    float *term_obs, int32_t auto_reset, void *stream)
{
    if (const int rc = finenv_host::ready(h, "step")) return rc;
    const finenv_host::DeviceGuard guard(h->device);
    if (!actions || !obs || !reward || !done)
        return finenv_host::fail(h, FINENV_ERR_INVALID, "step: null actions/obs/reward/done");
    BtParams p = bt_params(h);
    p.actions = actions;
    p.obs = obs;
    p.reward = reward;
    p.done = done;
    p.term_obs = term_obs;
    p.auto_reset = auto_reset;
    bt_launch<false>(p, (hipStream_t)stream);
    return finenv_host::check_launch(h, "btc_step");
}

}  // extern "C"
