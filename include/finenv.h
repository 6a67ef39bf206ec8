/*
 * finenv.h -- C ABI of libfinenv.so: MI355X-native batched trading environments.
 *
 * This is the drop-in boundary for the reference's market-environment hot path
 * (superyuri/FinRL, finrl/meta/env_stock_trading/env_stocktrading.py).  The reference
 * is pure Python, so there is no existing FFI to mirror symbol-for-symbol; each entry
 * point below names the reference method (file:line) whose work it replaces, and
 * INTEGRATION.md shows the ctypes binding a FinRL maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *   - Every buffer is CALLER-OWNED DEVICE memory (e.g. torch tensor .data_ptr());
 *     the library allocates nothing on the device and never synchronises the stream.
 *   - All launches go to the caller's hipStream_t, passed as void* (0 = null stream).
 *   - Return value: 0 = FINENV_OK, negative = error (finenv_strerror /
 *     finenv_stock_last_error).  No exceptions cross the ABI.
 *   - One handle per (device, stream) user; handles are thread-compatible, not
 *     thread-safe.
 *   - There is NO CPU fallback: without a HIP device every launch entry point fails
 *     with FINENV_ERR_HIP.
 *
 * Layout (E envs, N tickers, K indicators, T days, D = 1 + 2N + K*N)
 *   actions  [E][N] f32 row-major  (what SB3 / ElegantRL hand over)
 *   obs      [E][D] f32 row-major  = [cash | close[N] | holdings[N] | tech[K][N]]
 *                                    (indicator-major, env_stocktrading.py:456-467)
 *   state    structure-of-arrays over envs ([field][E] blocks); holdings is [N][E]
 *            (ticker-major) so that lane e of a wavefront reads holdings[i][e] coalesced.
 *   Limits   every device array must stay below 4 GiB (32-bit lane offsets).
 */
#ifndef FINENV_H
#define FINENV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FINENV_ABI_VERSION 3

enum {
    FINENV_OK = 0,
    FINENV_ERR_INVALID = -1,     /* bad argument / unsupported shape            */
    FINENV_ERR_UNBOUND = -2,     /* panel or state not bound yet                */
    FINENV_ERR_HIP = -3,         /* HIP runtime error (see *_last_error)        */
    FINENV_ERR_NOMEM = -4
};

#define FINENV_STOCK_MAX_TICKERS 128  /* two kernel variants: N <= 32 (DOW30), N <= 128
                                         (NASDAQ-100)                               */

/* Action domain of finenv_stock_step (stated here once; `hmax` below and the step's `actions` refer
 * to it).  An action is any finite f32: the reference does not clip, it trades
 * a = int(action * hmax) shares -- a float32 multiply, then truncation toward zero (:304-305) -- so
 * an action of 3.0 asks for 3 * hmax shares.  [-1, 1] is only the env's nominal action_space.  The
 * kernels do the same up to a SATURATION value of |a| that depends on the kernel stepping the batch
 * (a and the ticker index share one sort key):
 *     n_tickers <= 32                                 2^25
 *     n_tickers <= 128                                2^23
 *     n_tickers == 100 and hmax <= 255 (the NASDAQ-100 fast kernel: 16-bit sort keys)   255
 * Beyond it an action trades exactly as the saturated one does: same sign, same place in the trade
 * order among equally saturated actions (ticker order), never a wrapped value.  Inside it the step
 * equals the reference for every action, whatever binds the trade (the action, the holdings or
 * `cash // unit`, which is the exact floor division at every quotient).  Holdings are int32: keeping
 * them below 2^31 is the caller's business.  NaN and +-inf actions are unspecified (the reference's own
 * cast is undefined there); they trade some saturated or zero amount and never fault. */

/* Panel domain of finenv_stock_step (stated here once; finenv_stock_panel below refers to it).
 * Closes are finite and >= 0, at any magnitude: min(a, cash // unit) is the reference's at every
 * quotient (exact floor division below 2^40; beyond that the saturated action is always the smaller).
 * A close of 0 -- what FinRL's preprocessing writes for a missing price -- is a valid value:
 *   - a buy at close == 0 fills 0 shares and counts no trade (the reference divides by zero there:
 *     the one deliberate deviation);
 *   - a sell outside turbulence looks at the flag and the holdings only: at close == 0 it removes
 *     min(-a, held) shares, adds +0.0 to cash and cost and counts one trade (:105-129);
 *   - the turbulent liquidation sells a ticker only where close > 0 (:139-163): shares of a
 *     zero-priced ticker stay held, whatever its flag; a flagged ticker with close > 0 is sold.
 * The untradable flag is the fp64 compare tech_0 == 1.0 (:105, :174): neither fp64 neighbour of 1.0
 * is a flag, nor a value that only rounds to 1.0f in the observation.  It travels in the sign bit of
 * `close`, so a flagged zero close is -0.0 and an unflagged one +0.0; every valuation uses |close|.
 * An env is turbulent when turbulence >= turbulence_threshold (:308): equality liquidates, the next
 * double below does not, and with a threshold of 0.0 so do risk rows of +-0.0 and the 0 that reset()
 * leaves in `turbulence`.  NaN and +-inf closes, indicators and risk values are unspecified.
 * tests/test_gpu_stock_panel_domain.py holds every kernel to this. */

/* Constructor arguments of StockTradingEnv that shape the arithmetic
 * (env_stocktrading.py:24-47). */
typedef struct finenv_stock_config {
    int32_t n_envs;               /* E                                                   */
    int32_t n_tickers;            /* stock_dim, :50                                      */
    int32_t n_tech;               /* len(tech_indicator_list), :59                       */
    int32_t n_days;               /* len(df.index.unique()), :221                        */
    int32_t hmax;                 /* :51; at most 2^24 (N <= 32) or 2^22; int(action * hmax)
                                     saturates per kernel: see "Action domain" above       */
    int32_t use_turbulence;       /* turbulence_threshold is not None, :68               */
    int32_t reset_quirk;          /* 1: reset() builds obs from the row held before the
                                     rewind (reference behaviour, :361 vs :380-381)      */
    int32_t initial;              /* `initial` flag, :70 -- selects the summation order
                                     of asset_memory[0] (:364-378)                       */
    int32_t track_stats;          /* keep running sums of daily returns (Sharpe,
                                     :243-251) on device                                 */
    int32_t single_ticker;        /* 1 <=> len(df.tic.unique()) == 1 (needs n_tickers == 1):
                                     the reference's single-stock branches -- with `initial`
                                     the state starts from `[0] * stock_dim` shares whatever
                                     num_stock_shares holds (:415-422) while asset_memory[0]
                                     still counts them (:85-91, :364-370).  0 keeps the
                                     multi-stock rule for a 1-wide batch                   */
    double  buy_cost_pct;         /* scalar in this fork, :54                            */
    double  sell_cost_pct;        /* :55                                                 */
    double  reward_scaling;       /* :56                                                 */
    double  turbulence_threshold; /* :68                                                 */
} finenv_stock_config;

/* Read-only market panel (device pointers), packed by finrl_amd.panel.StockPanel from
 * the DataFrame the reference env receives (index = day ordinal, rows sorted by
 * (date, tic): preprocessors.py:24-33). */
typedef struct finenv_stock_panel {
    const double   *close;        /* [T][N]  fp64 closes: the money arithmetic runs on
                                     the same doubles the reference holds in state[1..N].
                                     The SIGN BIT of close[t][i] carries the day's
                                     "untradable" flag of ticker i: set <=> its first
                                     indicator == 1.0 on day t (the fork's `!= True` test,
                                     :105, :174, evaluated on the fp64 values); prices
                                     themselves are >= 0 by contract, 0 included (-0.0
                                     when flagged): see "Panel domain" above             */
    const float    *obs_tmpl;     /* [T][D]  f32 observation rows with the cash and
                                     holdings slots zero: f32(close) and f32(tech) in obs
                                     order (what DummyVecEnv's float32 buffer would hold) */
    const double   *risk;         /* [T]     df[risk_indicator_col], :337-341 (may be
                                     NULL when use_turbulence == 0)                      */
} finenv_stock_panel;

/* Mutable per-env state: two caller-owned device blocks of [field][env] arrays
 * (structure-of-arrays; lane e of a wavefront touches element e of every field, so every
 * access is coalesced, and two base pointers keep the kernels' scalar-register footprint
 * small).  Field order: */
enum {                            /* f64 block: double f64[FINENV_STOCK_F64_FIELDS][E]  */
    FINENV_SF_CASH = 0,           /* state[0]                                            */
    FINENV_SF_COST,               /* self.cost                                           */
    FINENV_SF_LAST_REWARD,        /* self.reward (scaled; survives reset)                */
    FINENV_SF_TURBULENCE,         /* self.turbulence                                     */
    FINENV_SF_ASSET0,             /* asset_memory[0] (written by init / reset only; the
                                     running asset_memory[-1] is never stored: it equals
                                     the next step's begin asset bit for bit)            */
    FINENV_SF_RET_SUM,            /* sum of pct_change(asset_memory) this episode        */
    FINENV_SF_RET_SUMSQ,          /* sum of its squares (Sharpe at the terminal step)    */
    FINENV_SF_CASH0,              /* initial_amount / previous_state[0] (read-only)      */
    FINENV_SF_BEGIN_ASSET,        /* cash + sum(close * shares) of the CURRENT observation,
                                     summed sequentially from ticker 0 as :311-314 does: the
                                     next step's begin_total_asset.  It is the previous step's
                                     end_total_asset bit for bit (same state list, same
                                     expression, :344-347), so step() carries it over instead
                                     of recomputing it; init / reset evaluate it afresh       */
    FINENV_STOCK_F64_FIELDS
};
enum {                            /* i32 block: int32 i32[FINENV_STOCK_I32_FIELDS+2N][E] */
    FINENV_SI_DAY = 0,            /* self.day                                            */
    FINENV_SI_PRICE_DAY,          /* row whose prices/indicators sit in the current
                                     observation (== day except right after a quirk
                                     reset)                                              */
    FINENV_SI_TRADES,             /* self.trades                                         */
    FINENV_SI_EPISODE,            /* self.episode                                        */
    FINENV_SI_START_DAY,          /* day the episode started on (init: day0, reset: 0;
                                     with windows s_e + day0 / s_e);
                                     daily returns accumulated so far = day - start_day  */
    FINENV_STOCK_I32_FIELDS       /* followed by holdings[N][E] = state[1+N .. 1+2N) and
                                     shares0[N][E] = num_stock_shares / previous_state
                                     shares (read-only)                                  */
};
typedef struct finenv_stock_state {
    double  *f64;                 /* [FINENV_STOCK_F64_FIELDS][E]                        */
    int32_t *i32;                 /* [FINENV_STOCK_I32_FIELDS + 2N][E]                   */
} finenv_stock_state;

typedef struct finenv_stock finenv_stock;   /* opaque host-side handle */

int         finenv_abi_version(void);
/* sizeof() of the ABI structs as the library was compiled (0 = finenv_stock_config,
 * 1 = finenv_stock_panel, 2 = finenv_stock_state, 3..5 = the finenv_portfolio_* trio, 6..8 = the finenv_crypto_* trio, 9..11 = the finenv_stocknp_* trio,
 * 12..14 = the finenv_cashpenalty_* trio, 15..17 = the finenv_stoploss_* trio, 19..21 = the finenv_btc_* trio,
 * 23 = finenv_replay_view, 24 = finenv_replay_batch, 26 = finenv_replay_nstep, 28 = finenv_replay_per,
 * 30 = finenv_rollout_view, 31 = finenv_rollout_batch, 33 = finenv_vecnorm; 22, 25, 27, 29 and 32, like 18, stay invalid as the ends of earlier lists):
 * lets a foreign-language binding verify its struct declarations at load time instead of corrupting
 * memory.  Index 18 stays FINENV_ERR_INVALID: it is what marked the end of the first v3 list, and
 * bindings probe it as such. */
int         finenv_struct_size(int which);
const char *finenv_strerror(int code);
/* Number of HIP devices visible, or a negative FINENV_ERR_HIP. */
int         finenv_device_count(void);

/* StockTradingEnv.__init__ (:24-100), config part.  Validates shapes. */
int  finenv_stock_create(const finenv_stock_config *cfg, finenv_stock **out);
void finenv_stock_destroy(finenv_stock *h);
const char *finenv_stock_last_error(const finenv_stock *h);
int  finenv_stock_obs_dim(const finenv_stock *h);

/* Row pitch, in floats, of the observation buffers later handed to step / reset / observe
 * (terminal observations stay packed).  Default = obs_dim (packed [E][D] rows, what the reference
 * returns); 0 restores it.  A pitch that is a multiple of 16 floats starts every row on a 64-byte
 * boundary: packed rows of 1204 B share their first and last 64-B segment with a neighbour that
 * is written ~13 us earlier or later (two partial HBM writes instead of one; PMC: 1.05x the bytes
 * stored).  The consumer sees a [E][D] view with a row stride. */
int  finenv_stock_set_obs_pitch(finenv_stock *h, int32_t pitch);

/* Performance hint, never needed for correctness: the envs of this batch may sit on different days
 * (per-env start days, episodes that end at different steps).  step() then launches the kernel
 * instantiation whose per-env panel-row paths are tuned (16-byte row copies, row-wise price gather,
 * parked head chunks); with every env on the same day -- the reference's training setup, BASELINE's
 * configs -- leave it off: that instantiation carries none of that code.
 * On a bound handle a call that flips the hint chooses the step kernel again and may query the device
 * (see finenv_stock_bind); before bind it only stores the value. */
int  finenv_stock_set_desync_hint(finenv_stock *h, int32_t on);

/* Attach the panel and state buffers (replaces self.df / self.state ownership).
 * Also decides how finenv_stock_step will launch: the kernel instantiation (from the config, the desync
 * hint and whether windows are attached) and how many blocks one launch takes (from the occupancy of
 * that kernel on the device that owns the state block).  bind, and finenv_stock_set_desync_hint /
 * finenv_stock_set_windows on a bound handle, may therefore query the device -- call them outside a
 * stream capture; finenv_stock_step never does: it only launches.  A second bind, possibly to a state
 * block on another device, decides again. */
int finenv_stock_bind(finenv_stock *h, const finenv_stock_panel *panel,
                      const finenv_stock_state *state);

/* __init__ state part (:64-91): every env starts on `day0` with cash0/shares0,
 * turbulence = cost = trades = episode = 0; no observation is produced
 * (use finenv_stock_observe). */
int finenv_stock_init(finenv_stock *h, int32_t day0, void *stream);

/* reset() (:359-393) for all envs, or those with mask[e] != 0 (device u8[E], may be
 * NULL).  Writes the reset observation rows into obs_out [E][D] (rows of unmasked envs
 * are left untouched). */
int finenv_stock_reset(finenv_stock *h, const uint8_t *mask, float *obs_out, void *stream);

/* render() / current state (:395-396): writes obs [E][D] without changing state. */
int finenv_stock_observe(finenv_stock *h, float *obs_out, void *stream);

/* After the CALLER has edited cash, holdings or price_day of the bound state block in place
 * (restoring a snapshot, desynchronising a batch): re-evaluate FINENV_SF_BEGIN_ASSET = cash +
 * sum(close[price_day] * holdings) in the reference's order (:311-314).  step() carries that field
 * from one step's end asset to the next step's begin asset and never recomputes it; init / reset
 * write it themselves.  Without this call the first reward after such an edit is computed against
 * a stale begin asset. */
int finenv_stock_refresh(finenv_stock *h, void *stream);

/* step() (:220-357) for all envs in ONE launch.
 *   actions   [E][N] f32, any finite value (nominally [-1, 1]): "Action domain" above
 *   obs       [E][D] f32 (next observation; after auto-reset: the reset observation)
 *   reward    [E]    f32 (float32 cast of the fp64 reward, as DummyVecEnv stores it)
 *   done      [E]    u8
 *   term_obs  [E][D] f32 or NULL: rows of envs with done == 1 receive the terminal
 *             observation (SB3 info["terminal_observation"]); other rows untouched
 *   realised  [E][N] i32 or NULL: shares actually traded (the values the reference
 *             writes back into `actions`, :324/:330 -> actions_memory)
 *   auto_reset != 0: envs that report done are reset inside the same launch
 *             (SB3 DummyVecEnv.step_wait semantics); 0: plain gym semantics (state
 *             unchanged on the terminal step, :301).
 */
int finenv_stock_step(finenv_stock *h, const float *actions, float *obs, float *reward,
                      uint8_t *done, float *term_obs, int32_t *realised, int32_t auto_reset,
                      void *stream);

/* Terminal-branch summary (:226-264) for every env, computed from current state:
 * out [E][6] f64 = {begin_total_asset, end_total_asset, total_reward, total_cost,
 *                   total_trades, sharpe (NaN if undefined)}. */
int finenv_stock_episode_stats(finenv_stock *h, double *out, void *stream);

/* Last-episode block: the summary of each env's most recently FINISHED episode, latched by the
 * step kernel on the step that reports done -- before an auto-reset replaces the state -- so that
 * it survives auto_reset != 0 (the reference prints it in the terminal step, :222-264, before
 * DummyVecEnv resets).  Opt-in and caller-owned: double last[FINENV_STOCK_LAST_FIELDS][E], device
 * memory, same [field][E] layout as the state blocks.  The library writes it only on done steps
 * (one write, and one COUNT increment, per reported done: with auto_reset == 0 every further
 * terminal step latches again, as the reference prints again); reset through the host does not
 * touch it.  The caller initialises it (COUNT = 0).  Fields: */
enum {
    FINENV_SL_COUNT = 0,          /* episodes finished since the block was enabled            */
    FINENV_SL_EPISODE,            /* self.episode of the finished episode                     */
    FINENV_SL_BEGIN_ASSET,        /* asset_memory[0]                                          */
    FINENV_SL_END_ASSET,          /* end_total_asset, :226-228                                */
    FINENV_SL_COST,               /* self.cost                                                */
    FINENV_SL_TRADES,             /* self.trades                                              */
    FINENV_SL_RET_N,              /* day - start_day: daily returns of the episode            */
    FINENV_SL_RET_SUM,            /* their sum (0 without track_stats)                        */
    FINENV_SL_RET_SUMSQ,          /* sum of their squares (0 without track_stats)             */
    FINENV_STOCK_LAST_FIELDS
};
/* Attach (or, with NULL, detach -- the default) a last-episode block.  The pointer is a step-kernel
 * argument: a step captured into a graph sees the block bound at capture time. */
int finenv_stock_set_last_episode(finenv_stock *h, double *last);
/* The episode_stats columns for the latched episodes: out [E][6] f64 = {begin_total_asset,
 * end_total_asset, total_reward, total_cost, total_trades, sharpe}; a row is all NaN while
 * COUNT == 0.  Sharpe is evaluated from the latched sums by the same code as episode_stats.
 * FINENV_ERR_INVALID when no block is attached. */
int finenv_stock_last_episode_stats(finenv_stock *h, double *out, void *stream);

/* Per-env episode windows: many data_split(df, dates[s], dates[t]) frames (preprocessors.py:24-33)
 * of ONE bound panel in one batch.  Opt-in and caller-owned: int32_t win[2][E], device memory;
 * win[0][e] = s_e (first panel row of env e's frame), win[1][e] = t_e (end, exclusive), and env e
 * then behaves like StockTradingEnv on that frame:
 *   - terminal when FINENV_SI_DAY >= t_e - 1 (:221);
 *   - a reset (host or auto) goes back to panel row s_e: FINENV_SI_DAY = FINENV_SI_START_DAY = s_e,
 *     the observation row is s_e (or, with reset_quirk, the row the env holds);
 *   - finenv_stock_init(day0) starts every env on row s_e + day0.
 * FINENV_SI_DAY stays the panel row; the reference's self.day is FINENV_SI_DAY - s_e.
 * Preconditions for a faithful result: 0 <= s_e < t_e <= n_days, and s_e + day0 < t_e at init.
 * The kernels clamp both rows into [0, n_days) whatever the block holds: a bad window is a wrong
 * answer, never an access outside the panel or the state.  Valid windows read no panel row
 * outside [s_e, t_e).
 * The pointer is a kernel argument (a graph captured after attaching sees later edits of the
 * block's CONTENTS).  step() reads t_e on every step and s_e only when it resets an env, so an
 * edited end applies from the next step and an edited start at the env's next reset.
 * NULL detaches (the default: every env runs rows 0 .. n_days-1).  Handle-wide settings (initial
 * amounts, costs) stay handle-wide.
 * Attaching or detaching on a bound handle (NULL <-> non-NULL) chooses the step kernel again and may
 * query the device (see finenv_stock_bind); another non-NULL pointer, or a call before bind, only
 * stores it. */
int finenv_stock_set_windows(finenv_stock *h, int32_t *win);

/* Episode history: asset_memory, date_memory and actions_memory (:85-97, :332, :348-349) of every
 * env's CURRENT episode, recorded on the device -- what save_asset_memory() / save_action_memory()
 * (:517-543), the account_value_*.csv of the terminal branch (:230-292) and get_validation_sharpe
 * read.  Opt-in and caller-owned device memory, time-major:
 *   asset[k][e]      the k-th entry of env e's asset_memory (fp64, the value the reference appends)
 *   row[k][e]        the panel row whose date is the k-th entry of its date_memory
 *   actions[k][e][:] the k-th entry of its actions_memory: the `realised` row of that step
 *   len[e]           entries recorded so far (actions: len[e] - 1); 0 = not armed, nothing is recorded
 *   flags[e]         FINENV_HIST_COMPLETE: the episode has reported done, the record is final;
 *                    FINENV_HIST_OVERFLOW: a step found len[e] == capacity and recorded nothing
 * While a history is attached, finenv_stock_step launches one more small kernel behind the step kernel
 * on the same stream (the step kernels themselves do not know about it).  Per env, by its own counter:
 *   - not armed (len == 0) or complete: nothing;
 *   - the step reported done: COMPLETE is set and nothing else is written -- the terminal branch
 *     appends to no memory (:222-301) -- whatever auto_reset is;
 *   - else entry k = len[e]: asset[k][e] = end_total_asset (:344-347), row[k][e] = FINENV_SI_DAY,
 *     actions[k-1][e][:] = realised[e][:], len[e] = k + 1; with k == capacity nothing is written and
 *     OVERFLOW is set.  No entry at or past `capacity` (actions: capacity - 1) is ever written.
 * Arming an env writes entry 0 -- what __init__ / reset() leave in the memories: asset_memory[0]
 * (FINENV_SF_ASSET0; with initial == 0 the previous total asset, :372-378) when the env stands at the
 * start of an episode, else its current total asset; its current FINENV_SI_DAY -- sets len[e] = 1 and
 * clears flags[e].  finenv_stock_init arms every env and finenv_stock_reset the envs it resets (the
 * reference's reset() wipes the lists).  An auto-reset inside step does NOT arm: the finished
 * episode's record stays readable and the env is not recorded again until a host reset or
 * finenv_stock_history_arm.  (DRL_prediction pulls the memories one step before the end because
 * DummyVecEnv's reset destroys them; here they survive it.)
 * The struct's pointers are LAUNCH ARGUMENTS: a step captured into a graph records only if the
 * history was attached before the capture, and into the tensors attached then.  With
 * actions != NULL, finenv_stock_step needs realised != NULL (FINENV_ERR_INVALID otherwise).
 * Memory: E * (12 * capacity + 8) + 4 * E * N * (capacity - 1) bytes. */
enum {
    FINENV_HIST_COMPLETE = 1,
    FINENV_HIST_OVERFLOW = 2
};
typedef struct finenv_stock_history {
    double  *asset;     /* [capacity][E]        asset_memory                              */
    int32_t *row;       /* [capacity][E]        panel row of date_memory                  */
    int32_t *actions;   /* [capacity-1][E][N]   actions_memory (realised), or NULL        */
    int32_t *len;       /* [E] entries recorded for the env's episode; 0 = not armed      */
    int32_t *flags;     /* [E] bit 0 complete, bit 1 overflow                             */
    int32_t  capacity;  /* >= 2                                                           */
} finenv_stock_history;
/* Attach a history (the struct is copied), or detach with NULL (the default).  Allowed before bind.
 * Attaching arms nothing: zero len / flags, then finenv_stock_init / _reset / _history_arm. */
int finenv_stock_set_history(finenv_stock *h, const finenv_stock_history *hist);
/* Arm every env, or those with mask[e] != 0 (device u8[E]), from its current state. */
int finenv_stock_history_arm(finenv_stock *h, const uint8_t *mask, void *stream);
/* Backtest figures of the recorded series: out [E][FINENV_STOCK_HISTORY_METRICS] f64, columns below;
 * daily returns r_k = asset[k] / asset[k-1] - 1, mean and std (ddof = 1) in two sequential passes as
 * pandas takes them.  sharpe = annualization * mean / std, NaN with fewer than two returns or
 * std == 0: annualization = sqrt(252) is the terminal printout (:243-251), sqrt(4) is
 * get_validation_sharpe.  Rows of unarmed envs are NaN. */
enum {
    FINENV_HM_N_RETURNS = 0,      /* len - 1                                                  */
    FINENV_HM_CUMULATIVE_RETURN,  /* asset[len-1] / asset[0] - 1                              */
    FINENV_HM_MEAN,               /* mean of the daily returns (NaN without one)              */
    FINENV_HM_STD,                /* their std, ddof = 1 (NaN with fewer than two)            */
    FINENV_HM_SHARPE,
    FINENV_HM_MAX_DRAWDOWN,       /* min_k (asset[k] / max_{j<=k} asset[j] - 1), <= 0         */
    FINENV_STOCK_HISTORY_METRICS
};
int finenv_stock_history_metrics(finenv_stock *h, double annualization, double *out, void *stream);

/* =====================================================================================
 * StockPortfolioEnv (finrl/meta/env_portfolio_allocation/env_portfolio.py:15-261)
 *   actions [E][N] f32 (portfolio scores; softmax-normalised inside, :225-229)
 *   obs     [E][D] f32, D = (N + K) * N: the day's N x N covariance rows then K indicator
 *           rows (:172-179) -- independent of per-env state
 *   reward  = new portfolio value, unscaled (:196-198)
 * Per-env state: portfolio_value, last reward (f64), day (i32).
 * ===================================================================================== */
/* Portfolio action and panel domain (stated here once; tests/test_gpu_portfolio_domain.py holds the
 * kernel to it).  The weights are the reference's softmax as written (:225-229), NOT a stabilised one:
 * float32 exp of every score, their float32 sum in NumPy's order (left to right below 8 terms, 8
 * accumulators combined pairwise from 8 on), one float32 division per weight.  No maximum is subtracted
 * and nothing is clamped, so what IEEE arithmetic makes of a score is the contract:
 *   - scores of any sign are fine; a score below about -87.3 has a subnormal exponential (coarse weights),
 *     one below about -104, or -inf, the exponential 0;
 *   - a score of 88.73 or more has the exponential +inf: that weight is inf / inf = NaN and every other
 *     weight of the env 0;
 *   - finite exponentials whose float32 sum exceeds FLT_MAX (two scores of 88.1, say) give weights that
 *     are all exactly 0: the portfolio return is 0 and the value stays what it was;
 *   - scores that all underflow (every one below about -104) give 0 / 0 = NaN in every weight.
 * A NaN weight makes the portfolio return and the value NaN.  So does the panel: a close of 0 gives the
 * return -1 into that day and +inf out of it (close[t+1] / 0), which is +inf in the value where the env
 * holds weight on the ticker and inf * 0 = NaN where its weight is exactly 0; two zero closes in a row
 * give 0 / 0 = NaN for every env.  A return of -1 held with weight exactly 1 leaves a value of exactly 0.
 * A value that is NaN or +-inf STAYS so on every further step (reward = float32 of it) until the env is
 * reset -- by finenv_portfolio_reset or by the auto-reset of its terminal step -- which restores
 * initial_amount.  done, day and the observation rows do not depend on the value and stay exact.
 * NaN and +inf scores are unspecified. */
#define FINENV_PORTFOLIO_MAX_TICKERS 64

typedef struct finenv_portfolio_config {
    int32_t n_envs;
    int32_t n_tickers;            /* stock_dim                                           */
    int32_t n_tech;               /* len(tech_indicator_list)                            */
    int32_t n_days;               /* len(df.index.unique()), :127                        */
    double  initial_amount;       /* :88, restored by reset() (:213)                     */
} finenv_portfolio_config;

typedef struct finenv_portfolio_panel {
    const double *gross_ret;      /* [T][N] f64: row t = close[t+1]/close[t] - 1, evaluated
                                     elementwise in fp64 exactly as :184 (row T-1 unused) */
    const float  *obs_tmpl;       /* [T][D] f32 observation rows                          */
} finenv_portfolio_panel;

enum { FINENV_PF_VALUE = 0, FINENV_PF_LAST_REWARD, FINENV_PORTFOLIO_F64_FIELDS };
enum { FINENV_PI_DAY = 0, FINENV_PORTFOLIO_I32_FIELDS };
typedef struct finenv_portfolio_state {
    double  *f64;                 /* [FINENV_PORTFOLIO_F64_FIELDS][E]                     */
    int32_t *i32;                 /* [FINENV_PORTFOLIO_I32_FIELDS][E]                     */
} finenv_portfolio_state;

typedef struct finenv_portfolio finenv_portfolio;

int  finenv_portfolio_create(const finenv_portfolio_config *cfg, finenv_portfolio **out);
void finenv_portfolio_destroy(finenv_portfolio *h);
const char *finenv_portfolio_last_error(const finenv_portfolio *h);
int  finenv_portfolio_obs_dim(const finenv_portfolio *h);
int  finenv_portfolio_bind(finenv_portfolio *h, const finenv_portfolio_panel *panel,
                           const finenv_portfolio_state *state);
/* reset() (:202-220) for all envs or those with mask[e] != 0; obs rows of reset envs. */
int  finenv_portfolio_reset(finenv_portfolio *h, const uint8_t *mask, float *obs_out,
                            void *stream);
/* step() (:125-200); weights_out [E][N] f32 or NULL receives the softmax weights
 * (actions_memory, :168); term_obs / auto_reset as in finenv_stock_step. */
int  finenv_portfolio_step(finenv_portfolio *h, const float *actions, float *obs, float *reward,
                           uint8_t *done, float *term_obs, float *weights_out,
                           int32_t auto_reset, void *stream);

/* Last-episode block of the portfolio env (same contract as the stock env's):
 * double last[FINENV_PORTFOLIO_LAST_FIELDS][E].  The state keeps no return history, so while a
 * block is attached every non-terminal step also adds its portfolio_return (:183-185) to RUN_SUM /
 * RUN_SUMSQ (16 B read + 16 B written per env); the terminal step latches them into RET_SUM /
 * RET_SUMSQ, and both the auto-reset and a host reset clear them.  The caller initialises COUNT = 0
 * and the running sums (0 for an env on day 0). */
enum {
    FINENV_PL_COUNT = 0,          /* episodes finished since the block was enabled            */
    FINENV_PL_BEGIN_VALUE,        /* asset_memory[0] = initial_amount                         */
    FINENV_PL_END_VALUE,          /* portfolio_value at the terminal step                     */
    FINENV_PL_RET_N,              /* len(portfolio_return_memory) = day + 1 (its leading 0
                                     included, :217)                                          */
    FINENV_PL_RET_SUM,            /* sum of portfolio_return_memory                           */
    FINENV_PL_RET_SUMSQ,          /* sum of its squares                                       */
    FINENV_PL_RUN_SUM,            /* running sums of the episode in progress                  */
    FINENV_PL_RUN_SUMSQ,
    FINENV_PORTFOLIO_LAST_FIELDS
};
int  finenv_portfolio_set_last_episode(finenv_portfolio *h, double *last);
/* out [E][3] f64 = {begin_total_asset, end_total_asset, sharpe} of the latched episodes (all NaN
 * while COUNT == 0); FINENV_ERR_INVALID when no block is attached. */
int  finenv_portfolio_last_episode_stats(finenv_portfolio *h, double *out, void *stream);

/* Per-env episode windows of the portfolio env (the contract of finenv_stock_set_windows):
 * many data_split(df, dates[s], dates[t]) frames of ONE bound panel in one batch.  Opt-in and
 * caller-owned: int32_t win[2][E], device memory; win[0][e] = s_e (first panel row of env e's
 * frame), win[1][e] = t_e (end, exclusive), and env e then behaves like StockPortfolioEnv on that
 * frame:
 *   - terminal when FINENV_PI_DAY >= t_e - 1 (:127);
 *   - a reset (host or auto, :202-220) goes back to panel row s_e: FINENV_PI_DAY = s_e and the
 *     observation row is s_e.
 * FINENV_PI_DAY stays the panel row; the reference's self.day is FINENV_PI_DAY - s_e.
 * Last-episode block: FINENV_PL_RET_N = FINENV_PI_DAY - s_e + 1, with s_e read at the terminal
 * step.  The state keeps no start day, so an edited start takes effect at that env's next reset;
 * an episode whose start was edited before it ended and that was never reset is out of contract
 * (set the new windows for the envs that just reported done, then reset them).
 * Preconditions for a faithful result: 0 <= s_e < t_e <= n_days.  The kernels clamp both rows
 * into [0, n_days) whatever the block holds: a bad window is a wrong answer, never an access
 * outside the panel or the state.  Valid windows read no panel row outside [s_e, t_e).
 * The pointer is a kernel argument: launches and graph replays see later edits of the block's
 * CONTENTS, but a graph keeps the pointer it was captured with.  step() reads t_e on every step
 * and s_e only when an env is terminal or reset, so an edited end applies from the next step and
 * an edited start at the env's next reset.  Works before bind.  NULL detaches (the default: every
 * env runs rows 0 .. n_days-1).  Returns FINENV_ERR_INVALID for a NULL handle. */
int  finenv_portfolio_set_windows(finenv_portfolio *h, int32_t *win);

/* Episode history of the portfolio env: asset_memory, portfolio_return_memory, date_memory and
 * actions_memory (:118-123, :168, :190-193) of every env's CURRENT episode, recorded on the device --
 * what save_asset_memory() / save_action_memory() (:231-252), DRL_prediction's two frames and the
 * terminal Sharpe (:145-153) read.  Opt-in and caller-owned device memory, time-major; all four
 * memories have the same length (actions_memory starts with the equal-weight row, :122):
 *   value[k][e]      the k-th entry of env e's asset_memory (fp64: the value the step stores to
 *                    FINENV_PF_VALUE)
 *   ret[k][e]        the k-th entry of its portfolio_return_memory (fp64: the step's own
 *                    portfolio_return, :183-185; entry 0 is the leading 0 of :121)
 *   row[k][e]        the panel row whose date is the k-th entry of its date_memory
 *   weights[k][e][:] the k-th entry of its actions_memory: the f32 softmax weights of that step
 *   len[e]           entries recorded so far; 0 = not armed, nothing is recorded
 *   flags[e]         FINENV_HIST_COMPLETE / FINENV_HIST_OVERFLOW, as in the stock env's history
 * portfolio_return is not in the state (the step folds it into the value and drops it), so the record
 * is taken INSIDE the step kernel: while a history is attached finenv_portfolio_step launches the
 * recording instantiation of its kernel, no second launch.  Per env, by its own counter:
 *   - not armed (len == 0) or complete: nothing;
 *   - the step is terminal for the env: COMPLETE is set and nothing else is written -- the terminal
 *     branch appends to no list (:130-156) -- whatever auto_reset is;
 *   - else entry k = len[e]: value[k][e] = the new portfolio_value (:193), ret[k][e] = this step's
 *     portfolio_return (:191), row[k][e] = the panel row the env moved to (:192), weights[k][e][:] =
 *     this step's softmax weights (:168), len[e] = k + 1; with k == capacity nothing is written and
 *     OVERFLOW is set.  No entry at or past `capacity` is ever written, in any tensor.
 * Arming an env writes entry 0 -- what __init__ / reset() leave in the memories: value[0][e] = its
 * current FINENV_PF_VALUE (the initial amount at the start of an episode), ret[0][e] = 0, row[0][e] =
 * its current FINENV_PI_DAY, weights[0][e][:] = (float)(1.0 / N) -- sets len[e] = 1 and clears
 * flags[e].  finenv_portfolio_reset arms the envs it resets (the reference's reset() wipes the lists,
 * :202-220).  An auto-reset inside step does NOT arm: the finished episode's record stays readable
 * and the env is not recorded again until a host reset or finenv_portfolio_history_arm.
 * (DRL_prediction pulls the memories one step before the end because DummyVecEnv's reset destroys
 * them; here they survive it.)
 * The struct's pointers are LAUNCH ARGUMENTS: a step captured into a graph records only if the
 * history was attached before the capture, and into the tensors attached then.
 * Memory: E * (20 * capacity + 8) + 4 * E * N * capacity bytes. */
typedef struct finenv_portfolio_history {
    double  *value;     /* [capacity][E]     asset_memory                                  */
    double  *ret;       /* [capacity][E]     portfolio_return_memory                       */
    int32_t *row;       /* [capacity][E]     panel row of date_memory                      */
    float   *weights;   /* [capacity][E][N]  actions_memory (softmax weights), or NULL     */
    int32_t *len;       /* [E] entries recorded for the env's episode; 0 = not armed       */
    int32_t *flags;     /* [E] FINENV_HIST_COMPLETE / FINENV_HIST_OVERFLOW                  */
    int32_t  capacity;  /* >= 2                                                            */
} finenv_portfolio_history;
/* Attach a history (the struct is copied), or detach with NULL (the default).  Allowed before bind.
 * Attaching arms nothing: zero len / flags, then finenv_portfolio_reset / _history_arm. */
int  finenv_portfolio_set_history(finenv_portfolio *h, const finenv_portfolio_history *hist);
/* Arm every env, or those with mask[e] != 0 (device u8[E]), from its current state. */
int  finenv_portfolio_history_arm(finenv_portfolio *h, const uint8_t *mask, void *stream);
/* Backtest figures of the recorded series: out [E][FINENV_STOCK_HISTORY_METRICS] f64, the FINENV_HM_*
 * columns, taken over the RECORDED returns ret[0 .. len-1] -- portfolio_return_memory with its leading
 * 0, what the terminal branch takes (:145-152) -- not over value ratios:
 *   N_RETURNS = len.  This differs from the stock env's len - 1 by that leading 0 (the convention
 *   of FINENV_PL_RET_N); CUMULATIVE_RETURN = value[len-1] / value[0] - 1; MEAN, STD (ddof = 1, NaN
 *   with fewer than two entries) in two sequential passes as pandas takes them; SHARPE =
 *   annualization * mean / std, NaN with fewer than two entries or std == 0 (the reference prints
 *   none then); MAX_DRAWDOWN over value.  Rows of unarmed envs are NaN. */
int  finenv_portfolio_history_metrics(finenv_portfolio *h, double annualization, double *out,
                                      void *stream);

/* =====================================================================================
 * CryptoEnv (finrl/meta/env_cryptocurrency_trading/env_multiple_crypto.py:10-111)
 *   actions [E][N] f32 in [-1,1], scaled per asset by the action normaliser (:63-65, :103-111)
 *   obs     [E][D] f32, D = 1 + N + W*lookback = [cash*2^-18 | stocks*2^-3 | tech[time-l]*2^-15]
 *   reward  (delta total asset) * 2^-16; on the last step the discounted return (:83-89)
 * Contract: price / tech arrays are float64 (as the reference's processors build them);
 * stocks are float32 (fractional), cash and assets float64.
 * ===================================================================================== */
#define FINENV_CRYPTO_MAX_ASSETS 32

typedef struct finenv_crypto_config {
    int32_t n_envs;
    int32_t n_assets;             /* crypto_num, :23                                     */
    int32_t n_tech;               /* tech_array.shape[1]                                 */
    int32_t n_steps;              /* price_array.shape[0]                                */
    int32_t lookback;             /* :13                                                 */
    int32_t reserved0;
    double  initial_cash;         /* initial_capital, :14-15                             */
    double  buy_cost_pct;         /* :16                                                 */
    double  sell_cost_pct;        /* :17                                                 */
    double  gamma;                /* :19                                                 */
} finenv_crypto_config;

/* Prices are finite and >= 0 (any magnitude: `cash // price` is the exact floor division).  A trade
 * needs price > 0, as in the reference (:67-77): at a price of 0 neither a sell nor a buy touches
 * holdings or cash, and the asset is valued at 0.  Row 0 must be > 0 throughout (action_norm_vector
 * takes its logarithm).  tests/test_gpu_crypto_panel_domain.py. */
typedef struct finenv_crypto_panel {
    const double *price;          /* [T][N] f64                                          */
    const float  *tech_scaled;    /* [T][W] f32 = float32(tech * 2^-15), :95-97          */
    const double *norm;           /* [N] action_norm_vector, :103-111 (host-evaluated)    */
} finenv_crypto_panel;

enum { FINENV_CF_CASH = 0, FINENV_CF_TOTAL_ASSET, FINENV_CF_GAMMA_RETURN,
       FINENV_CF_EPISODE_RETURN, FINENV_CF_LAST_REWARD, FINENV_CRYPTO_F64_FIELDS };
enum { FINENV_CI_TIME = 0, FINENV_CRYPTO_I32_FIELDS };
typedef struct finenv_crypto_state {
    double  *f64;                 /* [FINENV_CRYPTO_F64_FIELDS][E]                        */
    int32_t *i32;                 /* [FINENV_CRYPTO_I32_FIELDS][E]                        */
    float   *stocks;              /* [N][E] f32 holdings (fractional)                     */
} finenv_crypto_state;

typedef struct finenv_crypto finenv_crypto;

int  finenv_crypto_create(const finenv_crypto_config *cfg, finenv_crypto **out);
void finenv_crypto_destroy(finenv_crypto *h);
const char *finenv_crypto_last_error(const finenv_crypto *h);
int  finenv_crypto_obs_dim(const finenv_crypto *h);
int  finenv_crypto_bind(finenv_crypto *h, const finenv_crypto_panel *panel,
                        const finenv_crypto_state *state);
/* reset() (:48-57); gamma_return is NOT cleared, as in the reference. */
int  finenv_crypto_reset(finenv_crypto *h, const uint8_t *mask, float *obs_out, void *stream);
/* step() (:59-90).  The output pointers may address slice t of rollout tensors
 * [n_steps][E][...]: collecting a rollout needs no extra copy. */
int  finenv_crypto_step(finenv_crypto *h, const float *actions, float *obs, float *reward,
                        uint8_t *done, float *term_obs, int32_t auto_reset, void *stream);
/* step() that also records the policy's outputs of this step into the rollout tensors, in the same
 * launch (extra blocks beside the env blocks): actions -> actions_out [E][N], values -> values_out
 * [E], log_probs -> log_probs_out [E] (what SB3's RolloutBuffer.add copies; obs / reward / done are
 * written in place by the step itself).  All six buffers 16-byte aligned, E % 4 == 0, else
 * FINENV_ERR_INVALID (use finenv_crypto_step + finenv_rollout_put). */
int  finenv_crypto_step_record(finenv_crypto *h, const float *actions, float *obs, float *reward,
                               uint8_t *done, float *term_obs, int32_t auto_reset,
                               const float *values, const float *log_probs, float *actions_out,
                               float *values_out, float *log_probs_out, void *stream);

/* Per-env episode windows of the crypto env: many CryptoEnv instances built on slices
 * {'price_array': price[s:t], 'tech_array': tech[s:t]} of ONE bound panel in one batch (the
 * tutorial's train / test split, random-window training).  Env e on window [s_e, t_e) equals the
 * reference env on that slice; FINENV_CI_TIME stays the PANEL row (the reference's self.time is
 * FINENV_CI_TIME - s_e).  In panel rows:
 *   - a reset (finenv_crypto_reset or the auto-reset inside step) sets time = s_e + lookback - 1
 *     (:27, :49);
 *   - done when the incremented time equals t_e - lookback - 1 (:24, :80);
 *   - observation row l reads tech[time - l] as always; with a valid window no row outside
 *     [s_e, t_e) is read, and rows t_e - lookback .. t_e - 1 are never visited (as in the reference);
 *   - actions are scaled by the normaliser of row s_e, norm_rows[s_e][:] -- the reference derives
 *     action_norm_vector from price_array[0] of the array it was given (:103-111).
 * Only what the reference's reset() resets is reset: FINENV_CF_GAMMA_RETURN and _EPISODE_RETURN
 * survive (:48-57); a caller who wants "a fresh env object on a new slice" zeroes GAMMA_RETURN of
 * those envs.  A window needs t_e - s_e >= lookback + 2 (the n_steps rule of finenv_crypto_create).
 *
 * win: caller-owned device block int32_t [4][E], or NULL to detach (the default: every env runs
 * the whole panel with finenv_crypto_panel.norm).
 *   rows 0, 1  the PENDING window (s_e, t_e): the caller writes them whenever it likes, the env
 *              takes them at its next reset;
 *   rows 2, 3  the ACTIVE window of the running episode: written only by the reset paths
 *              (finenv_crypto_reset and the auto-reset inside step, which copy rows 0, 1 of the
 *              envs they reset), read by step.  Initialise them to the window of the episode in
 *              progress, or reset every env once after attaching.
 * Unlike the [2][E] blocks of the stock and portfolio envs: the crypto state has no start field
 * and the start stays live for the whole episode (it selects the normaliser), so an edit must
 * not reach a running episode.  With the two extra rows, redrawing the windows of the envs that
 * just reported done needs no reset launch: their auto-reset has already taken the windows that
 * were pending, the redraw is taken at the one after.
 * norm_rows: device f64 [n_steps][n_assets], one action normaliser per panel row; required while
 * win is non-NULL (FINENV_ERR_INVALID otherwise).  Rows whose prices are all positive hold
 * action_norm_vector(price[row]); a row with a price <= 0 holds NaN (the reference raises there):
 * a window that starts on such a row is out of contract and makes no trades.
 * The kernels clamp window rows and the rows they read into the panel whatever the block and the
 * time counter hold: bad device-side content is a wrong answer, never an access outside the panel.
 * Both pointers are kernel arguments: launches and graph replays see later edits of the block's
 * CONTENTS, a graph keeps the pointers it was captured with.  Works before bind.  Returns
 * FINENV_ERR_INVALID for a NULL handle. */
int finenv_crypto_set_windows(finenv_crypto *h, int32_t *win, const double *norm_rows);

/* Episode history of the crypto env: the account value of every env's CURRENT episode, one entry
 * per step, recorded on the device -- what DRLAgent.DRL_prediction_load_from_file
 * (agents/stablebaselines3/models.py:144-162) returns as episode_total_assets.  Opt-in and
 * caller-owned device memory, time-major:
 *   asset[k][e]      total_asset after the step (:82, :84): the step's own cash + sum, fp64
 *   holdings[k][e]   np.sum(stocks * price_array[time]) of that step (:82), NumPy's pairwise order:
 *                    the term the prediction loop builds its list from -- it appends
 *                    initial_total_asset + (price_array[time] * stocks).sum() (models.py:152-156),
 *                    not total_asset.  With both columns the true account value and the
 *                    reference's list can each be reproduced bit for bit.
 *   stocks[k][i][e]  holdings of asset i after the step (f32), or not recorded (NULL)
 *   start[e]         panel row of entry 0; entry k belongs to panel row start[e] + k
 *   len[e]           entries recorded so far; 0 = not armed, nothing is recorded
 *   flags[e]         FINENV_HIST_COMPLETE / FINENV_HIST_OVERFLOW, as in the stock env's history
 * Three choices differ from the portfolio env's struct:
 *   - no per-entry row: this env has no date_memory and its time counter advances by exactly one
 *     panel row per step, windows included, so one start row per env says everything (4 B per env
 *     and step saved);
 *   - holdings is recorded beside asset (above);
 *   - stocks is [capacity][N][E], the layout of the state's stocks tensor: a lane of the step kernel
 *     is an env, so every store of a wave is one contiguous 256 B ([E][N] would be strided here).
 * The holdings sum lives only in the step's registers, so the record is taken INSIDE the step
 * kernel: while a history is attached finenv_crypto_step / _step_record launch the recording
 * instantiation of their kernel, no second launch and no further dependent load.  Per env, by its
 * own counter:
 *   - not armed (len == 0) or complete: nothing;
 *   - else entry k = len[e]: asset[k][e] = the new total_asset, holdings[k][e] = the holdings sum,
 *     stocks[k][i][e] = the post-trade holdings (on a terminal step: before an auto-reset zeroes
 *     them), len[e] = k + 1; with k == capacity nothing is written and OVERFLOW is set.  No entry
 *     at or past `capacity` is ever written, in any tensor;
 *   - the terminal step IS recorded -- unlike the stock and portfolio envs this env trades and
 *     revalues on its last step (:59-90 has no terminal branch) -- and then sets COMPLETE, whatever
 *     auto_reset is (also when that step overflowed).
 * Arming an env writes entry 0 from its current state: asset[0][e] = FINENV_CF_TOTAL_ASSET,
 * holdings[0][e] = the same pairwise sum over the state's stocks and price[time] (exactly 0.0 at
 * the start of an episode, where asset[0] is exactly initial_cash), stocks[0][:][e] = the state's
 * holdings, start[e] = FINENV_CI_TIME; it sets len[e] = 1 and clears flags[e].
 * finenv_crypto_reset arms the envs it resets, behind the reset (with windows: on their new
 * active window).  An auto-reset inside step does NOT arm: the finished episode's record stays
 * readable and the env is not recorded again until a host reset or finenv_crypto_history_arm.
 * The struct's pointers are LAUNCH ARGUMENTS: a step captured into a graph records only if the
 * history was attached before the capture, and into the tensors attached then.
 * Memory: E * (16 * capacity + 12) + 4 * E * N * capacity bytes (262,144 envs on 1,440-row windows
 * of 10 pairs: 6 GB without stocks, 21 GB with -- which is why stocks is optional). */
typedef struct finenv_crypto_history {
    double  *asset;     /* [capacity][E]     total_asset after the step (:82, :84)                   */
    double  *holdings;  /* [capacity][E]     np.sum(stocks * price_array[time]) of that step (:82)  */
    float   *stocks;    /* [capacity][N][E]  holdings after the step, or NULL                        */
    int32_t *start;     /* [E] panel row of entry 0; entry k is panel row start[e] + k               */
    int32_t *len;       /* [E] entries recorded; 0 = not armed                                       */
    int32_t *flags;     /* [E] FINENV_HIST_COMPLETE / FINENV_HIST_OVERFLOW                            */
    int32_t  capacity;  /* >= 2                                                                      */
} finenv_crypto_history;
/* Attach a history (the struct is copied), or detach with NULL (the default).  Allowed before bind.
 * Attaching arms nothing: zero len / flags, then finenv_crypto_reset / _history_arm. */
int finenv_crypto_set_history(finenv_crypto *h, const finenv_crypto_history *hist);
/* Arm every env, or those with mask[e] != 0 (device u8[E]), from its current state. */
int finenv_crypto_history_arm(finenv_crypto *h, const uint8_t *mask, void *stream);
/* Backtest figures of the recorded account values: out [E][FINENV_STOCK_HISTORY_METRICS] f64, the
 * FINENV_HM_* columns with the stock env's convention: returns asset[k] / asset[k-1] - 1 for
 * k = 1 .. len-1, N_RETURNS = len - 1.  `annualization` is the caller's (one-minute bars have no
 * fixed year).  Rows of unarmed envs are NaN. */
int finenv_crypto_history_metrics(finenv_crypto *h, double annualization, double *out, void *stream);

/* =====================================================================================
 * Rollout helper (caller side of the path): generalized advantage estimation
 * over device-resident rollout tensors [n_steps][E], time-reverse scan, one lane per env.
 * Arithmetic follows stable-baselines3's documented RolloutBuffer.compute_returns_and_advantage
 * in float32 (SB3 is not vendored in the reference: parity unpinned, defined against the
 * documented formula):
 *   nnt_t   = 1 - dones[t]                 (dones[t] = done flag returned by step t)
 *   delta_t = rewards[t] + gamma * V_{t+1} * nnt_t - values[t],  V_{n} = last_values
 *   A_t     = delta_t + gamma * lam * nnt_t * A_{t+1};   returns_t = A_t + values[t]
 * ===================================================================================== */
int finenv_gae_scan(const float *rewards, const float *values, const uint8_t *dones,
                    const float *last_values, float *advantages, float *returns,
                    int32_t n_steps, int32_t n_envs, float gamma, float gae_lambda,
                    void *stream);

/* One launch that stores a policy's outputs for step t into the rollout tensors: actions [E][A],
 * values [E], log-probs [E] (float32, contiguous) -> the three destination slices.  Replaces the
 * three tensor copies of SB3's RolloutBuffer.add (its obs / reward / done parts need no copy: the
 * env kernels write them in place). */
int finenv_rollout_put(const float *actions, const float *values, const float *log_probs,
                       float *actions_out, float *values_out, float *log_probs_out,
                       int32_t n_envs, int32_t action_dim, void *stream);

/* Shuffled minibatches of a rollout (what SB3's RolloutBuffer.get(batch_size) yields, for PPO / A2C):
 * one launch per minibatch that draws its rows from a stateless permutation and gathers the six fields.
 *
 * Rows.  M = n_steps * n_envs, 1 <= M < 2^31; the flat row r = t * E + e of the time-major tensors
 *   obs [n_steps + 1][E][P] f32 (P = row pitch in floats >= D; slice n_steps, the observation after the
 *   last step, is never drawn), actions [n_steps][E][A], values / log_probs / advantages / returns
 *   [n_steps][E] f32.
 *
 * Permutation.  Position i in [0, M) of epoch n maps to row perm(i): a four-round Feistel network over
 * the bits of M - 1, cycle-walked into [0, M).  tests/rollout_model.py restates it.
 *   M == 1: the row is 0.  Otherwise bits = max(2, bit_length(M - 1)), a = bits / 2 (integer
 *   division), b = bits - a.  Split x into L = x >> a (b bits) and R = x & (2^a - 1), and for
 *   r = 0 .. 3:   even r:  L ^= F(R, r) & (2^b - 1);   odd r:  R ^= F(L, r) & (2^a - 1);
 *   F(h, r) = the first output word of Philox4x32-10 with counter (h, r, n lo, n hi) and key
 *   (seed lo, seed hi) -- the Philox of the replay draw below.  x' = L << a | R; while x' >= M the
 *   four rounds are applied again to x' (cycle walking).
 * Each round xors one half with a function of the other, so the rounds are a bijection of
 * [0, 2^bits); cycle walking restricts a bijection to one of [0, M) and ends, and as 2^bits < 2 M the
 * expected number of passes is below 2 (at M = 2^20 + 1 the longest walk of epochs 0, 1 and 5 under seed 7 takes 23 passes).
 * Uniformity: over 16,384 epochs at M = 48 and M = 80 every (position, row) count lies within 4.3
 * standard deviations of its mean.  For M < 16 a half holds one or two bits and the family of
 * permutations is visibly NOT uniform (M = 5: about 20 standard deviations off); a PPO buffer is never
 * that small.  The epoch number n is read from a device int64 the caller bumps in-stream, so a
 * captured epoch of minibatches plus that bump draws a fresh permutation at every replay.
 *
 * Gather.  Sample j of the batch is position i = first + j, r = perm(i):  observations[j] = obs row r
 * [:D] (columns D .. pitch-1 of the output are not written), actions[j] = actions row r, old_values[j]
 * = values[r], old_log_prob[j] = log_probs[r], advantages[j] = advantages[r], returns[j] = returns[r],
 * rows_out[j] = r.  8 D + 8 A + 36 bytes per sample with rows_out.  All offsets are 64-bit.  Rows move
 * in 16-byte pieces when D >= 4, P and the output pitch are multiples of 4 floats and the two
 * observation bases are 16-byte aligned, in dwords otherwise. */
typedef struct finenv_rollout_view {     /* finenv_struct_size 30 (29 stays invalid)            */
    const float *obs;                    /* [n_steps + 1][E][P]                                 */
    const float *actions;                /* [n_steps][E][A]                                     */
    const float *values;                 /* [n_steps][E]                                        */
    const float *log_probs;              /* [n_steps][E]                                        */
    const float *advantages;             /* [n_steps][E]                                        */
    const float *returns;                /* [n_steps][E]                                        */
    int32_t n_steps;                     /* >= 1                                                */
    int32_t n_envs;                      /* E >= 1; n_steps * E < 2^31                          */
    int32_t obs_dim;                     /* D >= 1                                              */
    int32_t obs_pitch;                   /* P >= D, floats                                      */
    int32_t action_dim;                  /* A >= 1                                              */
    int32_t reserved0;                   /* 0                                                   */
} finenv_rollout_view;

typedef struct finenv_rollout_batch {    /* finenv_struct_size 31 */
    float *observations;                 /* [B][pitch], columns 0 .. D-1 written                */
    float *actions;                      /* [B][A] packed                                       */
    float *old_values;                   /* [B]                                                 */
    float *old_log_prob;                 /* [B]                                                 */
    float *advantages;                   /* [B]                                                 */
    float *returns;                      /* [B]                                                 */
    int32_t batch_size;                  /* B >= 1                                              */
    int32_t obs_pitch;                   /* row pitch of observations, >= D                     */
} finenv_rollout_batch;

/* One launch: positions first .. first + B - 1 of the epoch in `*epoch` (device int64, read by the
 * kernel).  `first` and B are by value: first >= 0, first + B <= M.  rows_out: int32 [B] or NULL.
 * FINENV_ERR_INVALID, before any HIP call, for a null pointer, a dimension below 1, a pitch below
 * obs_dim, n_steps * n_envs >= 2^31 or broken bounds of first / B. */
int finenv_rollout_minibatch(const finenv_rollout_view *view, const int64_t *epoch, uint64_t seed,
                             int64_t first, const finenv_rollout_batch *batch, int32_t *rows_out,
                             void *stream);

/* =====================================================================================
 * Running observation / return statistics (what stable-baselines3's VecNormalize and RunningMeanStd
 * keep between a VecEnv and PPO / A2C / SAC; SB3 is not vendored in the reference: parity unpinned,
 * defined against the documented formulas, restated in tests/vecnorm_model.py).
 *
 * Stats block (caller-owned device memory, float64): mean[dim] and var[dim], starting at 0 and 1; one
 * count, starting at 1e-4; scale[d] = 1 / sqrt(var[d] + epsilon), stored so that applying takes no
 * division or square root per element.
 *
 * Update with a batch x of n rows: bm[d], bv[d] = the batch mean and POPULATION variance of column d,
 * then Chan's merge
 *   delta = bm - mean;  tot = count + n;  mean += delta * n / tot;
 *   var = (var * count + bv * n + delta^2 * count * n / tot) / tot;  count = tot;  scale recomputed.
 * The batch moments come from one read of x: rows are cut into at most FINENV_VECNORM_MAX_TILES tiles
 * of equal height (the last one ragged), each tile accumulates the float64 sums of (x - K) and
 * (x - K)^2 with K the tile's own first row -- never a plain sum of x^2, which loses the variance of a
 * column like 1e6 +- 1 to cancellation -- and the tiles' (n, mean, M2) merge by Chan's rule
 * (mean += delta * w, M2 += M2_b + delta^2 * w', w = n_b / tot, w' = n * n_b / tot) in a fixed order:
 * runs of consecutive tiles in tile order, then the runs in order.  The last block of the launch (one
 * ticket per block on `ticket`) does that merge and the one into the running stats, then resets the
 * ticket, so nothing waits, no floating-point atomic is used, and the same call on the same state gives
 * the same bits.  The tiling depends on (n_rows, dim) and on
 * whether rows move in 16-byte units (x 16-byte aligned, pitch a multiple of 4 floats, dim >= 4) or in
 * dwords; within one of those forms the result is a pure function of the data.
 * A NaN or an infinity in x stays in its own column: every other column gets the bits it would get
 * with a finite value in that cell.  The column itself ends with var = scale = NaN and a non-finite
 * mean, and stays so over later updates (apply then gives NaN in that column).  A NaN cell gives a NaN
 * mean.  For an infinite cell the mean depends on where the cell sits: as the first row of its tile it
 * is that tile's K, and inf - inf makes the mean NaN; elsewhere the tile's mean is that infinity, and
 * it survives the merge only in the last tile, since any tile merged after it adds (finite - inf) to it,
 * a NaN again; the next update does the same.
 *
 * Apply:  y = (double(x) - mean[d]) * scale[d];  y < -clip ? -clip : y > clip ? clip : y;  one rounding
 * to float32.  A NaN stays a NaN.  The subtract and the multiply round separately (the library builds
 * with -ffp-contract=off).  SB3 divides by sqrt(var + epsilon); multiplying by the stored reciprocal
 * differs from that by at most one rounding before the cast.  center = 0 drops the subtraction (the
 * reward form).  out == x with equal pitches works; columns dim .. pitch_out-1 are never written.
 * ===================================================================================== */
#define FINENV_VECNORM_MAX_TILES 128
typedef struct finenv_vecnorm {          /* finenv_struct_size 33 (32 stays invalid)            */
    double   *mean;                      /* [dim]                                               */
    double   *var;                       /* [dim]                                               */
    double   *scale;                     /* [dim]  1 / sqrt(var + epsilon)                      */
    double   *count;                     /* [1]                                                 */
    double   *partials;                  /* [partials_cap] scratch of an update launch          */
    uint32_t *ticket;                    /* one word, 0 between launches                        */
    int32_t   dim;                       /* >= 1                                                */
    int32_t   partials_cap;              /* doubles; 2 * FINENV_VECNORM_MAX_TILES * dim always
                                            suffices (an update needs 2 * tiles * dim)          */
    double    epsilon;
    double    clip;
} finenv_vecnorm;

/* scale[d] = 1 / sqrt(var[d] + epsilon) from the block's var (after the caller wrote mean / var /
 * count itself, e.g. loading saved statistics): one launch. */
int finenv_vecnorm_refresh(const finenv_vecnorm *stats, void *stream);

/* One launch: merge the n_rows x dim float32 batch x (rows `pitch` floats apart) into the stats.
 * FINENV_ERR_INVALID, before any launch, for a null pointer, dim < 1, n_rows < 1, pitch < dim or a
 * partials_cap too small for this launch. */
int finenv_vecnorm_update(const finenv_vecnorm *stats, const float *x, int64_t n_rows, int64_t pitch,
                          void *stream);

/* One launch: out[r][d] = apply(x[r][d]) for d < dim with the stats as they are.  center != 0: subtract
 * the mean; 0: scale and clip only.  Same refusals (pitch_in and pitch_out both >= dim). */
int finenv_vecnorm_apply(const finenv_vecnorm *stats, const float *x, int64_t n_rows, int64_t pitch_in,
                         float *out, int64_t pitch_out, int32_t center, void *stream);

/* VecNormalize.step_wait in SB3's order, for the [E, dim] observation and the reward / done of one env
 * step.  training != 0, two launches:
 *   1. update obs_stats with obs               2. obs_out = apply(obs) with the NEW stats
 *   3. returns[e] = returns[e] * gamma + reward[e]   (float64, * and + rounded separately)
 *   4. update ret_stats (dim 1) with returns   5. reward_out[e] = clip(double(reward[e]) * ret scale)
 *   6. returns[e] = 0 where done[e]
 * (1, 3, 4 in the first launch; 2, 5, 6 in the second).  training == 0: one launch, steps 2 and 5 only,
 * both stats blocks untouched.  norm_obs == 0 switches steps 1 and 2 off (obs_out is a copy of obs),
 * norm_reward == 0 steps 3 to 6 (reward_out is a copy of reward).  done_out: NULL, or uint8 [E] that
 * receives a copy of done in the last launch.  obs_out may be obs, reward_out may be reward.
 * FINENV_ERR_INVALID, before any launch, for a null struct or pointer (done_out apart), n_envs < 1,
 * a pitch below obs_stats->dim, ret_stats->dim != 1 or a partials_cap too small. */
int finenv_vecnorm_step(const finenv_vecnorm *obs_stats, const finenv_vecnorm *ret_stats,
                        const float *obs, int64_t obs_pitch, const float *reward, const uint8_t *done,
                        double *returns, double gamma, float *obs_out, int64_t obs_out_pitch,
                        float *reward_out, uint8_t *done_out, int32_t n_envs, int32_t training,
                        int32_t norm_obs, int32_t norm_reward, void *stream);

/* =====================================================================================
 * Replay buffer for the off-policy agents (DDPG / TD3 / SAC; the reference configures them with
 * buffer_size 50,000 .. 1,000,000 and batch_size 64 .. 128, finrl/config.py:41-50): a device-resident
 * ring the env kernels fill through their own output pointers, and a one-launch sampler.
 *
 * Ring (S slots, E envs, time-major, caller-owned):
 *   obs     [S][E][P] f32   P = row pitch in floats >= D; columns D .. P-1 are never read
 *   actions [S][E][A] f32
 *   rewards [S][E]    f32
 *   dones   [S][E]    u8
 * obs[s] is what the policy saw BEFORE the step stored in slot s; the next observation of slot s is
 * obs[(s+1) % S].  Every observation is stored once: the layout of stable-baselines3's
 * ReplayBuffer(optimize_memory_usage=True, handle_timeout_termination=False).
 *
 * Auto-reset.  The envs reset inside the step launch, so the next observation of a transition with
 * done == 1 is the FIRST observation of the next episode (what SB3 stores in that mode too).  The TD
 * target masks that row with 1 - done.  `done` is the reference's end of data (terminal =
 * day >= len(df.index.unique()) - 1, env_stocktrading.py:221): a time limit, which the reference's
 * agents nevertheless treat as termination -- so does this buffer.
 *
 * Head.  int32 head[2] = {pos, n_valid} in device memory: pos is the next slot to write, n_valid the
 * number of slots holding a complete transition, min(steps stored, S - 1); they are the slots
 * (pos - 1 - j) mod S for j in [0, n_valid).  Slot pos of a full ring is excluded: its observation
 * has been overwritten by the newest next observation (SB3: (randint(1, S) + pos) % S).  S >= 2.
 * finenv_replay_put SETS the head from by-value arguments (it never increments), so a replayed
 * capture publishes the head that belongs to the slots the capture writes; the sampler READS it from
 * device memory, so a captured sample sees the ring as it is at each replay.
 *
 * Draw.  Stateless and reproducible: Philox4x32-10 with key = (seed lo, seed hi) and counter =
 * (i, 0, draw lo, draw hi) for sample i; with the output words x0, x1:
 *   j = umulhi(x0, n_valid);  slot = (pos - 1 - j) mod S;  env = umulhi(x1, E).
 * The multiply-high map of a uniform 32-bit word onto [0, n) has a bias of at most n / 2^32 per
 * value (1.5e-5 at n = 65,536).  `draw` is read from a device int64 the caller bumps in-stream after
 * each sample, so a captured sample-plus-update graph draws fresh pairs at every replay.  Head words
 * are device data and are not trusted: n_valid < 1 is taken as 1, n_valid > S - 1 as S - 1, and the
 * slot is reduced mod S whatever pos holds -- bad words give wrong samples, never a fault.
 *
 * Gather.  For sample b = (s, e):  observations[b] = obs[s][e][:D];
 *   next_observations[b] = obs[(s+1) % S][e][:D];  actions[b] = actions[s][e];
 *   rewards[b] = rewards[s][e];  dones[b] = (float)dones[s][e].
 * Output columns D .. pitch-1 are not written.  All offsets are 64-bit: the 4 GiB limit of the env
 * arrays does not apply to the ring.  Rows move in 16-byte pieces when P and the output pitch are
 * multiples of 4 floats and the three bases are 16-byte aligned, in dwords otherwise.
 * ===================================================================================== */
typedef struct finenv_replay_view {      /* finenv_struct_size 23 */
    const float   *obs;                  /* [S][E][P]                                           */
    const float   *actions;              /* [S][E][A]                                           */
    const float   *rewards;              /* [S][E]                                              */
    const uint8_t *dones;                /* [S][E]                                              */
    int32_t n_slots;                     /* S >= 2                                              */
    int32_t n_envs;                      /* E >= 1                                              */
    int32_t obs_dim;                     /* D >= 1                                              */
    int32_t obs_pitch;                   /* P >= D, floats                                      */
    int32_t action_dim;                  /* A >= 1                                              */
    int32_t reserved0;                   /* 0                                                   */
} finenv_replay_view;

typedef struct finenv_replay_batch {     /* finenv_struct_size 24 */
    float *observations;                 /* [B][pitch], columns 0 .. D-1 written                */
    float *next_observations;            /* [B][pitch]                                          */
    float *actions;                      /* [B][A] packed                                       */
    float *rewards;                      /* [B]                                                 */
    float *dones;                        /* [B] 0.0f / 1.0f                                     */
    int32_t batch_size;                  /* B >= 1                                              */
    int32_t obs_pitch;                   /* row pitch of the two observation outputs, >= D      */
} finenv_replay_batch;

/* One launch: copy this step's actions (n_floats = E * A contiguous f32) into their ring slot and
 * store head[0] = pos_next, head[1] = n_valid_next (both >= 0).  `actions` may be the slot itself. */
int finenv_replay_put(const float *actions, float *actions_slot, int32_t n_floats, int32_t *head,
                      int32_t pos_next, int32_t n_valid_next, void *stream);

/* One launch: draw `batch->batch_size` (slot, env) pairs as stated above from the ring state in
 * `head` and the draw number in `*draw` (device int64), gather the five outputs, and, when
 * indices_out != NULL, store the pairs there as int32 [2][B] (row 0 slots, row 1 envs). */
int finenv_replay_sample(const finenv_replay_view *view, const int32_t *head, const int64_t *draw,
                         uint64_t seed, const finenv_replay_batch *batch, int32_t *indices_out,
                         void *stream);

/* One launch: the same gather for caller-supplied pairs, indices int32 [2][B] on the device (row 0
 * slots, row 1 envs; prioritised replay).  Slots are clamped into [0, S) and envs into
 * [0, E); whether a slot holds a complete transition is the caller's business. */
int finenv_replay_gather(const finenv_replay_view *view, const int32_t *indices,
                         const finenv_replay_batch *batch, void *stream);

/* n-step returns.  The same ring, head and draw; one launch that also walks each pair's reward /
 * done words forward.  For a start (s, e), n = n_steps and g = gamma:
 *
 * Horizon.  h = min(n, ((pos - 1 - s) mod S) + 1), mod non-negative: a start j slots behind the
 * newest stored step has j + 1 stored steps ahead of it (for the drawn pairs j is the draw's own j).
 * Every slot that is valid for the one-step sampler stays a valid start: a start too close to the
 * head yields a shorter return, it is not excluded.
 *
 * Length.  m is the smallest i in [1, h] with dones[(s+i-1) % S][e] != 0, or h if there is none.
 *
 * Return.  acc is a double; g_0 = 1.0f and g_{i+1} = g_i * g in one float32 multiply;
 *   acc = sum_{i=0}^{m-1} (double)g_i * (double)rewards[(s+i) % S][e], summed in increasing i
 * (the first term starts the sum);  rewards_out[b] = (float)acc.  The product of two floats is exact
 * in double, so the result does not depend on whether the compiler contracts the multiply-add, and
 * tests/replay_nstep_model.py states it bit for bit.  With n = 1 it is the stored reward, unchanged.
 *
 * Outputs.  dones_out[b] = (float)dones[(s+m-1) % S][e];  next_observations[b] =
 * obs[(s+m) % S][e][:D];  observations[b] and actions[b] are those of (s, e), as in the one-step
 * gather;  discounts[b] = g_m (float32): the caller's target is
 *   rewards + (1 - dones) * discounts * Q'(next_observations);
 * steps[b] = m (int32) when the pointer is not NULL.
 *
 * The draw is unchanged -- same Philox counter and key, same slot / env maps: for one (seed, draw
 * number, head), finenv_replay_sample_nstep returns the pairs finenv_replay_sample returns.
 *
 * Head words are untrusted, as above: every slot index is reduced mod S and n_valid is clamped as in
 * the one-step draw; bad words give wrong samples and never an address outside the ring.  In the
 * gather form slots and envs are clamped as finenv_replay_gather clamps them, and whether a slot is
 * a valid start is the caller's business.
 *
 * Arguments, checked on the host before any HIP call: 1 <= n_steps <= S - 1 (a window never comes
 * round to its own start), gamma finite and in [0, 1], head and discounts not NULL; anything else
 * returns FINENV_ERR_INVALID.  n_steps and gamma are by-value launch arguments: a captured call
 * keeps the values it was captured with. */
typedef struct finenv_replay_nstep {     /* finenv_struct_size 26 (25 stays invalid)            */
    const int32_t *head;                 /* {pos, n_valid}: read by both entry points           */
    float   *discounts;                  /* [B] g_m                                             */
    int32_t *steps;                      /* [B] m, or NULL                                      */
    int32_t n_steps;                     /* 1 .. S - 1                                          */
    float   gamma;                       /* [0, 1]                                              */
} finenv_replay_nstep;

/* One launch each, on the caller's stream, nothing allocated, no synchronisation: the n-step forms
 * of finenv_replay_sample and finenv_replay_gather.  The sample form reads its `head` argument for
 * the draw and the horizon alike; the gather form reads nstep->head.  The struct is checked by one
 * rule in both forms (head not NULL): a caller passes the same pointer twice. */
int finenv_replay_sample_nstep(const finenv_replay_view *view, const int32_t *head,
                               const int64_t *draw, uint64_t seed, const finenv_replay_batch *batch,
                               const finenv_replay_nstep *nstep, int32_t *indices_out, void *stream);
int finenv_replay_gather_nstep(const finenv_replay_view *view, const int32_t *indices,
                               const finenv_replay_batch *batch, const finenv_replay_nstep *nstep,
                               void *stream);

/* Prioritised replay.  Per-transition priorities beside the ring, a sum tree kept consistent on the
 * device, a proportional draw fused into the sampler's launch (one-step and n-step) and the priority
 * write-back.  Everything is integer, so nothing depends on summation order and
 * tests/replay_per_model.py restates it exactly.
 *
 * Tickets.  A priority is stored as an unsigned 32-bit fixed-point ticket.  For a shaped priority w
 * (float32, the caller's (|delta| + eps)^alpha -- the powers stay with the caller: powf is not
 * bit-reproducible) and F = frac_bits in [0, 31]:
 *   q = 1                                          if !(w > 0)   (NaN, zero, negatives)
 *   q = min(max(rint((double)w * 2^F), 1), 2^32 - 1)   otherwise (exact in double; ties to even)
 * so a stored transition always has q >= 1 and stays drawable, and q == 0 means, and only means,
 * "this slot holds no complete transition".  The resolution floor is 2^-F: a priority below it draws
 * as if it were 2^-F.  Leaves are tickets[S][E] in the ring's order, leaf = s * E + e, N = S * E
 * <= 2^31 - 1.
 *
 * Tree.  Fan-out 64.  Level 1 has n_1 = ceil(N / 64) nodes over the leaves, level k has
 * ceil(n_{k-1} / 64); the last level is the one with a single node.  Every node is the exact uint64
 * sum of its children; children past the end count as 0.  Levels are stored top-down: tree[0] is the
 * root (the total), then the level below it, and so on; level 1 comes last.  N <= 64 is one word;
 * N = 4617 is 1 + 2 + 73 = 76 words.
 *
 * Selection.  With c = the inclusive prefix sums of the tickets in leaf order, a value u in
 * [0, total) selects the one leaf with c[leaf-1] <= u < c[leaf] (NumPy: searchsorted(c, u,
 * side="right")): never a leaf at 0.  u >= total is taken as total - 1; total == 0 gives pair (0, 0).
 *
 * Validity lives in the tickets: the prioritised draw does not read n_valid.  When a step is stored
 * in slot pos (finenv_replay_per_put), the E leaves of slot pos take *max_ticket (a value of 0 is
 * taken as 1) -- new transitions enter at the largest priority seen -- and the E leaves of slot
 * pos_next take 0: its observation has just been overwritten (the slot the uniform draw excludes by
 * the head rule).  Unfilled slots are 0 from allocation.
 *
 * Draw.  For sample i the Philox4x32-10 counter (i, 0, draw lo, draw hi) and key of the uniform
 * draw; with its first two words x = (x0 << 32) | x1 and u = umul64hi(x, total), the leaf is selected
 * as above and the outputs are gathered exactly as finenv_replay_gather gathers them (n-step: by the
 * n-step rule above, unchanged, the horizon measured from nstep->head).
 * probabilities_out[b] = (float)((double)q / (double)total), q the leaf's ticket; may be NULL.
 *
 * Tree words are device data and are not trusted: the descent clamps the child to 63 and every index
 * to its level, the leaf to N - 1.  A tree that disagrees with its leaves gives wrong samples, never
 * an address outside the ring.
 *
 * Every entry point takes the caller's stream, allocates nothing, does not synchronise and is a fixed
 * number of launches that depends only on (S, E): one per tree level for rebuild; one plus one per
 * level above the first for put and update; one for find and for each sample form.  Arguments are
 * checked on the host before any HIP call: NULL pointers, frac_bits outside [0, 31], S < 2, E < 1,
 * S * E > 2^31 - 1, batch_size < 1, pos or pos_next outside [0, S) return FINENV_ERR_INVALID. */
typedef struct finenv_replay_per {       /* finenv_struct_size 28 (27 stays invalid)            */
    uint32_t *tickets;                   /* [S][E] leaves                                       */
    uint64_t *tree;                      /* finenv_replay_per_tree_words(S * E) words           */
    uint32_t *max_ticket;                /* one device word; a value of 0 is taken as 1         */
    int32_t   frac_bits;                 /* 0 .. 31                                             */
    int32_t   reserved0;                 /* 0                                                   */
} finenv_replay_per;

/* Host only: the words of the tree over n_leaves leaves; -1 for n_leaves < 1 or > 2^31 - 1. */
int64_t finenv_replay_per_tree_words(int64_t n_leaves);

/* Make every node the sum of its children from the leaves as they are (restoring state). */
int finenv_replay_per_rebuild(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs,
                              void *stream);

/* The fill rule above for the step stored in slot pos, by value like finenv_replay_put, and the sums
 * repaired.  pos_next == pos zeroes nothing. */
int finenv_replay_per_put(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs, int32_t pos,
                          int32_t pos_next, void *stream);

/* The write-back.  indices int32 [2][B] (clamped as finenv_replay_gather clamps), weights float32 [B]
 * (shaped priorities w).  A leaf at 0 stays 0: an update for an excluded or unfilled slot is dropped;
 * any other leaf takes its entry's ticket.  *max_ticket = max(*max_ticket, every entry's ticket),
 * dropped entries included.  Afterwards every node equals the sum of its children.  Duplicate
 * indices with different weights: the leaf ends as one of them, unspecified which, and the tree is
 * still consistent with the leaves (the sampler's own duplicates are the same transition and
 * normally carry the same value). */
int finenv_replay_per_update(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs,
                             const int32_t *indices, const float *weights, int32_t batch_size,
                             void *stream);

/* The descent alone: u uint64 [B] on the device -> the pairs of the selected leaves, int32 [2][B]
 * (for a caller with its own, e.g. stratified, u). */
int finenv_replay_per_find(const finenv_replay_per *per, int32_t n_slots, int32_t n_envs,
                           const uint64_t *u, int32_t batch_size, int32_t *indices_out, void *stream);

/* One launch each: draw, descend, gather (S and E are the view's).  probabilities_out float32 [B] or
 * NULL; indices_out int32 [2][B] or NULL.  The n-step form reads nstep->head for the horizon. */
int finenv_replay_per_sample(const finenv_replay_view *view, const finenv_replay_per *per,
                             const int64_t *draw, uint64_t seed, const finenv_replay_batch *batch,
                             float *probabilities_out, int32_t *indices_out, void *stream);
int finenv_replay_per_sample_nstep(const finenv_replay_view *view, const finenv_replay_per *per,
                                   const int64_t *draw, uint64_t seed,
                                   const finenv_replay_batch *batch, const finenv_replay_nstep *nstep,
                                   float *probabilities_out, int32_t *indices_out, void *stream);

/* =====================================================================================
 * Array-state StockTradingEnv (finrl/meta/env_stock_trading/env_stocktrading_np.py:8-169),
 * the ElegantRL / RLlib-facing env.
 *   actions [E][N] f32;  obs [E][D] f32, D = 3 + 3N + W =
 *     [amount*2^-12 | turbulence_ary[d] | turbulence_bool[d] | price*2^-6 | stocks*2^-6 |
 *      cool_down | tech_ary[d]]                                               (:149-162)
 *   reward = delta total_asset * reward_scaling; discounted return on the last step (:137-145)
 * Numerics: bit-identical to the reference under NumPy >= 2 (NEP 50), where amount /
 * total_asset / gamma_reward are Python-float, float32 or float64 depending on the trade
 * history; the dtype of each is tracked per env (FINENV_NT_*, 2 bits each in the `tags` word)
 * and every operation is performed in the dtype NumPy would use.
 * ===================================================================================== */
#define FINENV_STOCKNP_MAX_TICKERS 32
enum { FINENV_NT_PY = 0, FINENV_NT_F32 = 1, FINENV_NT_F64 = 2 };

typedef struct finenv_stocknp_config {
    int32_t n_envs;
    int32_t n_tickers;
    int32_t n_techw;              /* tech_ary.shape[1] (= N*K, ticker-major)              */
    int32_t n_days;               /* price_ary.shape[0]; max_step = n_days - 1, :67       */
    int32_t min_action;           /* int(max_stock * min_stock_rate), :111                */
    int32_t reserved0;
    double  max_stock;            /* :39 (action scale, :104)                             */
    double  buy_cost_pct, sell_cost_pct, reward_scaling, gamma;
    double  obs_amount_floor;     /* 0: the observation shows self.amount (:150); > 0: Python's
                                     max(self.amount, floor) as StockEnvNAS100.get_state does
                                     (env_nas100_wrds.py:154, floor = 1e4)                 */
} finenv_stocknp_config;

/* Action domain of finenv_stocknp_step.  An action is any finite f32: the reference does not clip, it
 * trades a = (actions * max_stock).astype(int) shares (:104) -- the product taken in float32, then truncated
 * toward zero -- so an action of 3.0 asks for 3 * max_stock shares and |action * max_stock| < 1 for none.
 * [-1, 1] is only the env's nominal action_space.  Both compares against min_action are strict (:112,
 * :120): a == +-min_action trades nothing, and with min_action == 0 a == +-1 trades.  Both min() calls
 * return their first, float32, operand at equality: min(stocks[i], -a) with -a == stocks[i] sells on the
 * float32 product chain, min(amount // price, a) at equality buys the quotient, and the dtype tag the env
 * carries from then on follows (:114, :124).  `amount // price` is NumPy's: the exact floor in float64 and,
 * for a float32 amount, what npy_floor_dividef returns -- the floor below 2^22, its two float32 roundings
 * from there on.
 * For |trunc(action * max_stock)| <= S = 2^31 - 128, the largest float32 an int32 holds, the step equals
 * the reference exactly, whatever binds the trade.  Beyond S an action trades exactly as +-S does: same
 * sign, never a wrapped value (the reference's int64 would ask for more; holdings and cash cut both short
 * alike unless more than S shares are there to sell or to pay for).  NaN and +-inf actions are unspecified
 * (the reference's own cast is undefined there); they trade some amount within +-S and never fault.
 * tests/test_gpu_stocknp_action_domain.py holds the kernel to this. */

/* Prices are finite f32 >= 0.  A trade needs price > 0, as in the reference (:112-129): at a price of
 * 0 neither a sell nor a buy touches holdings, amount or the cool-down, which goes on counting; the
 * turbulent liquidation (:131-134) sells everything and values a zero-priced holding at 0.  A day is
 * turbulent when turbulence > thresh (:32): equality is calm.  tests/test_gpu_stocknp_panel_domain.py. */
typedef struct finenv_stocknp_panel {
    const float *price;           /* [T][N] price_ary (f32), :27                          */
    const float *obs_tmpl;        /* [T][D] f32 rows: turbulence / price*2^-6 / tech filled,
                                     amount, stocks and cool_down slots zero              */
    const float *turb_bool;       /* [T]    (turbulence > thresh) as f32, :32             */
} finenv_stocknp_panel;

enum { FINENV_NF_AMOUNT = 0, FINENV_NF_TOTAL_ASSET, FINENV_NF_GAMMA_REWARD,
       FINENV_NF_INITIAL_TOTAL_ASSET, FINENV_NF_EPISODE_RETURN, FINENV_NF_LAST_REWARD,
       FINENV_NF_AMOUNT0, FINENV_STOCKNP_F64_FIELDS };
enum { FINENV_NI_DAY = 0, FINENV_NI_TAGS, FINENV_NI_AMOUNT0_TAG, FINENV_STOCKNP_I32_FIELDS };
/* tags word: bits 0-1 amount, 2-3 total_asset, 4-5 gamma_reward, 6-7 initial_total_asset,
 * 8-9 last reward */
typedef struct finenv_stocknp_state {
    double  *f64;                 /* [FINENV_STOCKNP_F64_FIELDS][E]                       */
    int32_t *i32;                 /* [FINENV_STOCKNP_I32_FIELDS][E]                       */
    float   *f32;                 /* [3N][E]: stocks[N], cool_down[N], stocks0[N]          */
} finenv_stocknp_state;

typedef struct finenv_stocknp finenv_stocknp;

int  finenv_stocknp_create(const finenv_stocknp_config *cfg, finenv_stocknp **out);
void finenv_stocknp_destroy(finenv_stocknp *h);
const char *finenv_stocknp_last_error(const finenv_stocknp *h);
int  finenv_stocknp_obs_dim(const finenv_stocknp *h);
/* row pitch (floats) of the obs buffers of step / reset; see finenv_stock_set_obs_pitch */
int  finenv_stocknp_set_obs_pitch(finenv_stocknp *h, int32_t pitch);
int  finenv_stocknp_bind(finenv_stocknp *h, const finenv_stocknp_panel *panel,
                         const finenv_stocknp_state *state);
/* reset() (:80-101) from the per-env start state (stocks0, amount0, amount0_tag): eval mode =
 * (initial_stocks, initial_capital as FINENV_NT_PY); train mode = caller-drawn values with
 * FINENV_NT_F32 (the reference draws them from the global numpy RNG, :85-92). */
int  finenv_stocknp_reset(finenv_stocknp *h, const uint8_t *mask, float *obs_out, void *stream);
int  finenv_stocknp_step(finenv_stocknp *h, const float *actions, float *obs, float *reward,
                         uint8_t *done, float *term_obs, int32_t auto_reset, void *stream);

/* Per-env episode windows of the array-state env: many StockTradingEnv / StockEnvNAS100 instances
 * built on slices {'price_array': price[s:t], 'tech_array': tech[s:t], 'turbulence_array':
 * turb[s:t]} of ONE bound panel in one batch (the train / test date ranges of finrl/train.py and
 * finrl/test.py, random-window training).  The constructor's array preparation (:27-35) is
 * elementwise, so the bound panel, the template rows and turb_bool stay as they are.  Env e on
 * window [s_e, t_e) equals the reference env on that slice, bit for bit; FINENV_NI_DAY stays the
 * PANEL row (the reference's self.day is FINENV_NI_DAY - s_e).  In panel rows:
 *   - a reset (finenv_stocknp_reset or the auto-reset inside step) sets day = s_e, restores
 *     stocks / cool-downs / amount from the start state, total_asset = amount +
 *     (stocks * price[s_e]).sum() in the same float32 pairwise order, gamma_reward = 0, and shows
 *     observation row s_e (:80-101);
 *   - a step increments day, trades at price[day] under turb_bool[day] and is done when the
 *     incremented day equals t_e - 1 (:67, :142); FINENV_NF_EPISODE_RETURN is latched as always;
 *   - with a valid window no panel row outside [s_e, t_e) is read.
 * A window needs t_e - s_e >= 2 (the n_days rule of finenv_stocknp_create).  The start state
 * (stocks0, amount0, amount0_tag) is the caller's as before: a train-mode draw (:85-92) depends on
 * price[s_e], the first row of the env's slice.
 *
 * win: caller-owned device block int32_t [4][E], or NULL to detach (the default: every env runs
 * the whole panel).
 *   rows 0, 1  the PENDING window (s_e, t_e): the caller writes them whenever it likes, the env
 *              takes them at its next reset;
 *   rows 2, 3  the ACTIVE window of the running episode: written only by the reset paths
 *              (finenv_stocknp_reset for the envs it selects and the auto-reset inside step, which
 *              copy rows 0, 1 of the envs they reset), read by step.  Initialise them to the
 *              window of the episode in progress, or reset every env once after attaching.
 * The crypto env's layout, not the [2][E] blocks of the stock and portfolio envs: the end row is
 * read on every step, so an edit must not reach a running episode.  With the two extra rows,
 * redrawing the windows of the envs that just reported done needs no reset launch (and works
 * inside a captured graph): their auto-reset has already taken the windows that were pending, the
 * redraw is taken at the one after.
 * The kernels clamp window rows and the day counter into the panel whatever the block and the
 * state hold: bad device-side content is a wrong answer, never an access outside the panel or
 * the state.
 * The pointer is a kernel argument: launches and graph replays see later edits of the block's
 * CONTENTS, a graph keeps the pointer it was captured with.  Works before bind.  Returns
 * FINENV_ERR_INVALID for a NULL handle. */
int finenv_stocknp_set_windows(finenv_stocknp *h, int32_t *win);

/* Episode history of the array-state env: the account curve of every env's CURRENT episode, one
 * entry per step, recorded on the device -- what DRLAgent.DRL_prediction
 * (agents/elegantrl/models.py:105-131) returns as episode_total_assets: the env's total_asset after
 * every step.  Opt-in and caller-owned device memory, time-major:
 *   asset[k][e]      total_asset after the step (:137), the value as the state holds it (fp64; a
 *                    float32 total_asset is that float32 widened)
 *   tag[k][e]        FINENV_NT_* of that total_asset -- the NumPy-2 scalar type the reference's list
 *                    holds at that position (Python float / np.float32 / np.float64) -- or not
 *                    recorded (NULL)
 *   stocks[k][i][e]  holdings of ticker i after the step (f32), or not recorded (NULL)
 *   start[e]         panel row of entry 0; entry k belongs to panel row start[e] + k
 *   len[e]           entries recorded so far; 0 = not armed, nothing is recorded
 *   flags[e]         FINENV_HIST_COMPLETE / FINENV_HIST_OVERFLOW, as in the stock env's history
 * As in the crypto env's struct there is no per-entry row -- the day counter advances by exactly one
 * panel row per step, windows included -- and stocks is [capacity][N][E], the layout of the state's
 * books: a lane of the step kernel is an env, so every store of a wave is one contiguous 256 B.
 * Under auto_reset the step overwrites FINENV_NF_TOTAL_ASSET with the restarted episode's value in
 * the launch that computed the terminal one, so the record is taken INSIDE the step kernel: while a
 * history is attached finenv_stocknp_step launches the recording instantiation of its kernel, no
 * second launch and no further dependent load on the trading wave.  Per env, by its own counter:
 *   - not armed (len == 0) or complete: nothing;
 *   - else entry k = len[e]: asset[k][e] = the step's new total_asset, before any auto-reset touches
 *     it, tag[k][e] = its dtype tag, stocks[k][i][e] = the post-trade holdings (on a turbulence day:
 *     the zeros), len[e] = k + 1; with k == capacity nothing is written and OVERFLOW is set.  No
 *     entry at or past `capacity` is ever written, in any tensor;
 *   - the terminal step IS recorded -- this env trades and revalues on its last step (:103-147 has
 *     no terminal branch) -- and then sets COMPLETE, whatever auto_reset is (also when that step
 *     overflowed).
 * Arming an env writes entry 0 from its current state: asset[0][e] = FINENV_NF_TOTAL_ASSET,
 * tag[0][e] = bits 2-3 of the tags word, stocks[0][:][e] = the state's holdings, start[e] =
 * FINENV_NI_DAY (the panel row, windows included); it sets len[e] = 1 and clears flags[e].
 * finenv_stocknp_reset arms the envs it resets, behind the reset (with windows: on their new active
 * window; in train mode: on the drawn start state).  An auto-reset inside step does NOT arm: the
 * finished episode's record stays readable and the env is not recorded again until a host reset or
 * finenv_stocknp_history_arm.
 * The struct's pointers are LAUNCH ARGUMENTS: a step captured into a graph records only if the
 * history was attached before the capture, and into the tensors attached then.
 * Memory: E * (9 * capacity + 12) + 4 * E * N * capacity bytes (65,536 envs on 504-row windows of the
 * DOW30: 0.3 GB without stocks, 4.3 GB with -- which is why stocks is optional). */
typedef struct finenv_stocknp_history {
    double  *asset;     /* [capacity][E]    total_asset after the step (:137), value as the state holds it */
    uint8_t *tag;       /* [capacity][E]    FINENV_NT_* of that total_asset (NumPy-2 scalar dtype), or NULL */
    float   *stocks;    /* [capacity][N][E] holdings after the step, or NULL                                */
    int32_t *start;     /* [E] panel row of entry 0; entry k is panel row start[e] + k                      */
    int32_t *len;       /* [E] entries recorded; 0 = not armed                                              */
    int32_t *flags;     /* [E] FINENV_HIST_COMPLETE / FINENV_HIST_OVERFLOW                                  */
    int32_t  capacity;  /* >= 2                                                                             */
} finenv_stocknp_history;
/* Attach a history (the struct is copied), or detach with NULL (the default).  Allowed before bind.
 * Attaching arms nothing: zero len / flags, then finenv_stocknp_reset / _history_arm. */
int finenv_stocknp_set_history(finenv_stocknp *h, const finenv_stocknp_history *hist);
/* Arm every env, or those with mask[e] != 0 (device u8[E]), from its current state. */
int finenv_stocknp_history_arm(finenv_stocknp *h, const uint8_t *mask, void *stream);
/* Backtest figures of the recorded account values: out [E][FINENV_STOCK_HISTORY_METRICS] f64, the
 * FINENV_HM_* columns with the stock env's convention: returns asset[k] / asset[k-1] - 1 in fp64 for
 * k = 1 .. len-1, N_RETURNS = len - 1.  Rows of unarmed envs are NaN. */
int finenv_stocknp_history_metrics(finenv_stocknp *h, double annualization, double *out, void *stream);

/* =====================================================================================
 * StockTradingEnvCashpenalty
 * (finrl/meta/env_stock_trading/env_stocktrading_cashpenalty.py:19-409): continuous (or
 * discretised) share counts from dollar-sized actions, no per-ticker ordering, reward =
 * (assets - cash-shortfall penalty) / initial - 1, per elapsed step (:237-247); episode ends at
 * the last date or on a cash shortage (unless patient) (:333-344).
 *   actions [E][N] f32;  obs [E][D] f32, D = 1 + N + N*C = [cash | holdings | info[N][C]]
 * Contract: scalar hmax.  The three dot products per step are summed left to right
 * (the reference uses BLAS ddot, order unspecified: agreement ~1e-15 relative).
 *
 * Panel domain.  Closes are finite and > 0, at any magnitude.  The reference divides by the close
 * unguarded (:276, :286): at close == 0 its continuous form yields NaN holdings and its discrete form
 * the platform's integer cast of a NaN, so a zero close is outside the domain here (the kernel then
 * sells the holdings of that asset: unspecified, no fault).  Discrete actions: integer share
 * counts from `act * hmax // close` (:263-274), which is NumPy's floor_divide and not floor(a / close)
 * (3.0 // 0.1 == 29); the kernel's division is that one for |act * hmax / close| < 2^50.  Equality at
 * a compare is decided as the reference decides it: turbulence == turbulence_threshold liquidates
 * (`>=`, :282), spend + costs == cash is no shortage (`>`, :333: the step is applied and cash lands on
 * 0.0), total * cash_penalty_proportion == cash is no penalty (:241).  NaN and +-inf closes and risk
 * values are unspecified.  tests/test_gpu_cashpenalty_panel_domain.py holds every launch form to this.
 * ===================================================================================== */
#define FINENV_CASHPENALTY_MAX_ASSETS 32

typedef struct finenv_cashpenalty_config {
    int32_t n_envs, n_assets, n_cols, n_days;
    int32_t discrete_actions;     /* :60, :263-274                                        */
    int32_t shares_increment;     /* :61                                                  */
    int32_t use_turbulence;       /* turbulence_threshold is not None, :282               */
    int32_t patient;              /* :68, :334-339                                        */
    double  hmax;                 /* :59 (dollars per trade)                              */
    double  buy_cost_pct, sell_cost_pct, initial_amount, cash_penalty_proportion,
            turbulence_threshold;
} finenv_cashpenalty_config;

typedef struct finenv_cashpenalty_panel {
    const double *close;          /* [T][N] f64                                           */
    const float  *info;           /* [T][N*C] f32 date vectors, ticker-major (:159-171)   */
    const double *turb;           /* [T] f64 (may be NULL when use_turbulence == 0)       */
} finenv_cashpenalty_panel;

enum { FINENV_KF_COH = 0, FINENV_KF_TURBULENCE, FINENV_KF_SUM_TRADES, FINENV_KF_LOGGED_TOTAL,
       FINENV_KF_LOGGED_CASH, FINENV_CASHPENALTY_F64_FIELDS /* then holdings[N][E] */ };
enum { FINENV_KI_DATE_INDEX = 0, FINENV_KI_START, FINENV_KI_EPISODE,
       FINENV_KI_NEXT_START,      /* starting point the next reset() uses (random_start: the
                                     caller refills it; the reference draws it with `random`).
                                     A panel row; with a window block attached
                                     (finenv_cashpenalty_set_windows) an OFFSET from the first
                                     row of the env's pending window, clamped into the window */
       FINENV_CASHPENALTY_I32_FIELDS };
typedef struct finenv_cashpenalty_state {
    double  *f64;                 /* [FINENV_CASHPENALTY_F64_FIELDS + N][E]                */
    int32_t *i32;                 /* [FINENV_CASHPENALTY_I32_FIELDS][E]                    */
} finenv_cashpenalty_state;

typedef struct finenv_cashpenalty finenv_cashpenalty;

int  finenv_cashpenalty_create(const finenv_cashpenalty_config *cfg, finenv_cashpenalty **out);
void finenv_cashpenalty_destroy(finenv_cashpenalty *h);
const char *finenv_cashpenalty_last_error(const finenv_cashpenalty *h);
int  finenv_cashpenalty_obs_dim(const finenv_cashpenalty *h);
int  finenv_cashpenalty_bind(finenv_cashpenalty *h, const finenv_cashpenalty_panel *panel,
                             const finenv_cashpenalty_state *state);
int  finenv_cashpenalty_reset(finenv_cashpenalty *h, const uint8_t *mask, float *obs_out,
                              void *stream);
/* random_start (:134-138: `random.choice(range(int(len(dates) * 0.5)))`): with hi > 0 every reset
 * (explicit or inside step) draws its starting point on the device, uniformly in [0, hi), from a
 * counter-based generator keyed by (seed, env, episode) -- no host work per step; hi == 0 (default):
 * resets take FINENV_KI_NEXT_START.  Not bit-reproducible against Python's `random` by construction.
 * With a window block attached (finenv_cashpenalty_set_windows) only the sign of hi is read: env e
 * draws in [0, max(1, (t_e - s_e) >> 1)) of the window [s_e, t_e) it is reset onto -- the same
 * int(len(self.dates) * 0.5) on the env's own slice -- and starts on panel row s_e + draw. */
int  finenv_cashpenalty_set_random_start(finenv_cashpenalty *h, int32_t hi, uint64_t seed);
int  finenv_cashpenalty_step(finenv_cashpenalty *h, const float *actions, float *obs,
                             float *reward, uint8_t *done, float *term_obs, int32_t auto_reset,
                             void *stream);
/* Harness log (the reference's account_information / transaction_memory lists, :149-154, :345-347,
 * read back by save_asset_memory / save_action_memory :382-409): when `audit` is non-NULL every
 * step writes one f64 row [FINENV_AUDIT_HEAD + N] per env:
 *   begin cash (:307/:312), asset value (:310), reward in f64 (:317), reason flags, then the N
 *   transactions that were (or, on a cash-shortage terminal step, would have been) applied.
 * Meant for the single-env facades (back-tests); NULL (default) = no log, no extra traffic. */
enum { FINENV_AUDIT_BEGIN_CASH = 0, FINENV_AUDIT_ASSET_VALUE, FINENV_AUDIT_REWARD,
       FINENV_AUDIT_FLAGS, FINENV_AUDIT_HEAD };
enum { FINENV_AUDIT_F_LAST_DATE = 1, FINENV_AUDIT_F_CASH_SHORTAGE = 2,
       FINENV_AUDIT_F_TURBULENCE = 4, FINENV_AUDIT_F_STOP_LOSS = 8,
       FINENV_AUDIT_F_LOW_PROFIT = 16, FINENV_AUDIT_F_HIGH_PROFIT = 32 };
int  finenv_cashpenalty_set_audit(finenv_cashpenalty *h, double *audit /* [E][HEAD+N] or NULL */);

/* Per-env episode windows of the cash-penalty env: many StockTradingEnvCashpenalty instances built
 * on the frame restricted to dates[s:t] (self.dates, the cached date vectors and closings of that
 * slice) of ONE bound panel in one batch -- train / trade splits, ensemble validation windows,
 * random-window collection.  Env e on window [s_e, t_e) equals the reference env on that slice, with
 * the tolerance the env has without windows; FINENV_KI_DATE_INDEX and FINENV_KI_START stay PANEL
 * rows (the reference's date_index is FINENV_KI_DATE_INDEX - s_e; current_step =
 * FINENV_KI_DATE_INDEX - FINENV_KI_START as always).  In panel rows:
 *   - the episode ends at the window's last date, date_index == t_e - 1 (:299), or on a cash
 *     shortage as always; FINENV_AUDIT_F_LAST_DATE means the window's last date;
 *   - a reset (finenv_cashpenalty_reset or the auto-reset inside step) starts the env
 *       with random_start on (hi > 0): on s_e + draw, the draw of (seed, env, episode) in
 *         [0, max(1, (t_e - s_e) >> 1)) -- the per-window draw range; only the sign of hi is read;
 *       otherwise: on s_e + clamp(FINENV_KI_NEXT_START, 0, t_e - s_e - 1) -- NEXT_START is an
 *         OFFSET from the window's first row;
 *   - with a valid window no row of close, info or turb outside [s_e, t_e) is read, the streamer's
 *     speculative copy of the next row included.
 * A window needs t_e - s_e >= 1 (the n_days rule of finenv_cashpenalty_create); the first step of a
 * one-row window ends at the last date.
 *
 * win: caller-owned device block int32_t [4][E], or NULL to detach (the default: every env runs
 * the whole panel, and everything behaves as without this call).
 *   rows 0, 1  the PENDING window (s_e, t_e): the caller writes them whenever it likes, the env
 *              takes them at its next reset;
 *   rows 2, 3  the ACTIVE window of the running episode: written only by the reset paths
 *              (finenv_cashpenalty_reset for the envs it selects and the auto-reset inside step,
 *              which copy rows 0, 1 of the envs they reset), read by step (row 3).  Initialise
 *              them to the window of the episode in progress, or reset every env once after
 *              attaching.
 * The layout of the crypto and array-state envs, not the [2][E] blocks of the stock and portfolio
 * envs: the end row is read on every step by both waves of the step kernel, so an edit must not
 * reach a running episode, and the random_start draw range depends on the window, so a reset must
 * see both rows together.  With the two extra rows, redrawing the windows of the envs that just
 * reported done needs no reset launch (and works inside a captured graph): their auto-reset has
 * already taken the windows that were pending, the redraw is taken at the one after.
 * The kernels clamp window rows (s into [0, T - 1], t into [s + 1, T]) and the date index into the
 * panel whatever the block and the state hold: bad device-side content is a wrong answer, never an
 * access outside the panel or the state.
 * The pointer is a kernel argument: launches and graph replays see later edits of the block's
 * CONTENTS, a graph keeps the pointer it was captured with.  Works before bind.  Returns
 * FINENV_ERR_INVALID for a NULL handle. */
int  finenv_cashpenalty_set_windows(finenv_cashpenalty *h, int32_t *win);

/* =====================================================================================
 * StockTradingEnvStopLoss
 * (finrl/meta/env_stock_trading/env_stocktrading_stoploss.py:19-459): the cash-penalty env
 * plus an average-buy-price book per asset: positions are force-sold when
 * close < stoploss_penalty * avg_buy_price (and cash >= stoploss_penalty * initial, :353-357);
 * the reward adds a stop-loss penalty, a low-profit penalty and a profit bonus (:255-290).
 * Quirks kept (see oracle/stoploss_oracle.c): per-step reward uses the PREVIOUS step's
 * logged totals (:313 precedes :315-318); the turbulence sell-off goes through
 * (h*close)/close (:330,:345); patient mode still books the cancelled buys (:376 vs :418).
 *   actions [E][N] f32;  obs [E][D] f32, D = 1 + N + N*C  (same layout as the cash-penalty env)
 *
 * Panel domain.  Closes are finite and >= 0, at any magnitude, and 0 means "missing data" as in the
 * reference, which guards every division with close > 0 (:326, :335, :345): a request at close == 0
 * trades nothing, whatever its sign, the turbulent sell-off -(h * 0) is a transaction of 0 that keeps
 * the asset held, and neither counts in actual_num_trades (:411).  The stop-loss itself looks at no
 * price guard (:350-357): closing_diff_avg_buy = 0 - stoploss_penalty * avg_buy_price < 0 for a held
 * asset, so an armed env gives such a position away at 0.0, as the reference does.  Discrete actions:
 * `a // close` (:335) is NumPy's floor_divide, not floor(a / close), and the kernel's division is that
 * one for |act * hmax / close| < 2^50.  Equality at a compare is decided as the reference decides
 * it: turbulence == threshold liquidates (`>=`, :329); cash == stoploss_penalty * initial_amount arms the
 * stop-loss (`>=`, :353); closing_diff_avg_buy == 0 forces no sale (`<`, :356); spend + costs == cash is
 * no shortage (`>`, :372); a sale at close == avg_buy_price is no profit (`>`, :392); holdings of
 * exactly 0 clear the buy book (`>`, :427).  NaN and +-inf closes and risk values are unspecified.
 * tests/test_gpu_stoploss_panel_domain.py holds every launch form to this.
 * ===================================================================================== */
#define FINENV_STOPLOSS_MAX_ASSETS 32

typedef struct finenv_stoploss_config {
    int32_t n_envs, n_assets, n_cols, n_days;
    int32_t discrete_actions;     /* :71, :333-343                                        */
    int32_t shares_increment;     /* :72                                                  */
    int32_t use_turbulence;       /* turbulence_threshold is not None, :327-331           */
    int32_t patient;              /* :373-378                                             */
    double  hmax;                 /* :70 (scalar)                                         */
    double  buy_cost_pct, sell_cost_pct, initial_amount, cash_penalty_proportion,
            turbulence_threshold;
    double  stoploss_penalty;     /* :73                                                  */
    double  min_profit_penalty;   /* 1 + profit_loss_ratio * (1 - stoploss_penalty), :101 */
} finenv_stoploss_config;

typedef struct finenv_stoploss_panel {
    const double *close;          /* [T][N] f64                                           */
    const float  *info;           /* [T][N*C] f32 date vectors, ticker-major (:167-180)   */
    const double *turb;           /* [T] f64 (may be NULL when use_turbulence == 0)       */
} finenv_stoploss_panel;

enum { FINENV_LF_COH = 0, FINENV_LF_TURBULENCE, FINENV_LF_SUM_TRADES, FINENV_LF_LOGGED_TOTAL,
       FINENV_LF_LOGGED_CASH, FINENV_LF_ACTUAL_NUM_TRADES, FINENV_STOPLOSS_F64_FIELDS };
/* after the scalar rows, six [N][E] f64 books in this order */
enum { FINENV_LV_HOLDINGS = 0, FINENV_LV_PREV_HOLDINGS, FINENV_LV_CLOSING_DIFF_AVG_BUY,
       FINENV_LV_PROFIT_SELL_DIFF_AVG_BUY, FINENV_LV_N_BUYS, FINENV_LV_AVG_BUY_PRICE,
       FINENV_STOPLOSS_BOOKS };
enum { FINENV_LI_DATE_INDEX = 0, FINENV_LI_START, FINENV_LI_EPISODE,
       FINENV_LI_NEXT_START,      /* as FINENV_KI_NEXT_START: a panel row, or with a window block
                                     attached an offset from the pending window's first row */
       FINENV_STOPLOSS_I32_FIELDS };

typedef struct finenv_stoploss_state {
    double  *f64;                 /* [FINENV_STOPLOSS_F64_FIELDS + FINENV_STOPLOSS_BOOKS*N][E] */
    int32_t *i32;                 /* [FINENV_STOPLOSS_I32_FIELDS][E]                           */
} finenv_stoploss_state;

typedef struct finenv_stoploss finenv_stoploss;

int  finenv_stoploss_create(const finenv_stoploss_config *cfg, finenv_stoploss **out);
void finenv_stoploss_destroy(finenv_stoploss *h);
const char *finenv_stoploss_last_error(const finenv_stoploss *h);
int  finenv_stoploss_obs_dim(const finenv_stoploss *h);
int  finenv_stoploss_bind(finenv_stoploss *h, const finenv_stoploss_panel *panel,
                          const finenv_stoploss_state *state);
/* reset(), :134-165 (mask NULL = all envs; starting points from FINENV_LI_NEXT_START) */
int  finenv_stoploss_reset(finenv_stoploss *h, const uint8_t *mask, float *obs_out, void *stream);
/* step(), :292-442 (+ DummyVecEnv auto-reset when auto_reset != 0) */
/* as finenv_cashpenalty_set_random_start (:142-147), the per-window draw range with a window block
 * attached included */
int  finenv_stoploss_set_random_start(finenv_stoploss *h, int32_t hi, uint64_t seed);
int  finenv_stoploss_step(finenv_stoploss *h, const float *actions, float *obs, float *reward,
                          uint8_t *done, float *term_obs, int32_t auto_reset, void *stream);
/* as finenv_cashpenalty_set_audit; flags additionally carry STOP_LOSS (:359-360) and
 * LOW_PROFIT / HIGH_PROFIT (:401-405), the reasons the reference logs for this env */
int  finenv_stoploss_set_audit(finenv_stoploss *h, double *audit /* [E][HEAD+N] or NULL */);

/* Per-env episode windows of the stop-loss env: the contract of finenv_cashpenalty_set_windows, word
 * for word, with StockTradingEnvStopLoss on the frame restricted to dates[s:t], FINENV_LI_* for
 * FINENV_KI_* and "last date" at :302.  win is the same caller-owned device block int32_t [4][E] --
 * rows 0, 1 the PENDING window, rows 2, 3 the ACTIVE one, written only by finenv_stoploss_reset for
 * the envs it selects and by the auto-reset inside step -- or NULL to detach (the default).  The
 * per-window draw range of random_start, FINENV_LI_NEXT_START as an offset from the window's first
 * row and the clamping of window rows and date index are the same (one implementation,
 * finenv_twowave.h).  The pointer is a kernel argument: graph replays see later edits of the
 * block's contents, a graph keeps the pointer it was captured with.  Works before bind.  Returns
 * FINENV_ERR_INVALID for a NULL handle. */
int  finenv_stoploss_set_windows(finenv_stoploss *h, int32_t *win);

/* Episode history of the cash-penalty and stop-loss envs: what the reference keeps in
 * account_information, actions_memory and transaction_memory (env_stocktrading_cashpenalty.py:308-355,
 * env_stocktrading_stoploss.py:315-385) and hands out through save_asset_memory() /
 * save_action_memory(), for every env's CURRENT episode, recorded on the device.  Opt-in and
 * caller-owned device memory, time-major:
 *   cash[k][e], asset_value[k][e], reward[k][e], reason[k][e]
 *                          the audit head of the k-th recorded step: begin cash, asset value, the f64
 *                          reward, the FINENV_AUDIT_F_* reason flags (total_assets is cash + asset_value,
 *                          formed by the reader as the reference forms it)
 *   transactions[k][e][:]  the N transactions of that step (f64), or not recorded (NULL)
 *   actions[k][e][:]       the raw f32 action row finenv_<kind>_step was given, or not recorded (NULL)
 *   start[e]               panel row of entry 0; entry k belongs to panel row start[e] + k
 *   end[e]                 end of the window the record was armed on (n_days without windows): the
 *                          reference's `date` column is the last len dates of the env's own frame
 *   ntx[e]                 transaction rows the reference's list holds: len[e], or one fewer when the
 *                          episode ended on a cash shortage (it returns before the append, :341-344)
 *   len[e]                 entries recorded so far; 0 is a legal armed record (the lists are empty
 *                          after reset())
 *   flags[e]               FINENV_HIST_ARMED | FINENV_HIST_COMPLETE | FINENV_HIST_OVERFLOW
 * The record is a copy of the audit row, so a history needs the audit block
 * (finenv_<kind>_set_audit): while a history is attached finenv_<kind>_step launches one more small
 * kernel behind the step kernel on the same stream (the step kernels do not know about it) and
 * returns FINENV_ERR_INVALID, "history needs an audit block", without one.  Per env that is armed
 * and not complete, from the audit row the step left and its done[e]:
 *   - flags contain FINENV_AUDIT_F_LAST_DATE: nothing is appended (:299-301), COMPLETE is set;
 *   - else len[e] == capacity: OVERFLOW is set, nothing is written; COMPLETE too if done[e];
 *   - else entry k = len[e]: the four scalars, the action row, and the transactions unless the step
 *     ended the episode on a cash shortage (CASH_SHORTAGE and done[e]); len[e] = k + 1, ntx[e]
 *     counts the transaction rows; COMPLETE if done[e].
 *   No entry at or past `capacity` is ever written, in any tensor.
 * Arming an env sets len = ntx = 0, flags = ARMED, start[e] = its current FINENV_KI_DATE_INDEX and
 * end[e] = its active window's end.  finenv_<kind>_reset arms the envs it resets, behind the reset.
 * An auto-reset inside step does NOT arm: the finished episode's record stays readable and the env
 * is not recorded again until a host reset or finenv_<kind>_history_arm.
 * The struct's pointers are LAUNCH ARGUMENTS: a step captured into a graph records only if the
 * history was attached before the capture, and into the tensors attached then.
 * Memory: E * (28 * capacity + 20) + 12 * E * N * capacity bytes with both optional tensors. */
enum { FINENV_HIST_ARMED = 4 };    /* beside FINENV_HIST_COMPLETE / _OVERFLOW; these two envs only */
typedef struct finenv_twowave_history {
    double  *cash;          /* [capacity][E]    begin cash of the step (:312)                       */
    double  *asset_value;   /* [capacity][E]    asset value (:310)                                  */
    double  *reward;        /* [capacity][E]    the f64 reward (:317)                               */
    int32_t *reason;        /* [capacity][E]    FINENV_AUDIT_F_* flags of the step                  */
    double  *transactions;  /* [capacity][E][N] transaction_memory, or NULL                         */
    float   *actions;       /* [capacity][E][N] the raw action rows, or NULL                        */
    int32_t *start;         /* [E] panel row of entry 0; entry k is panel row start[e] + k          */
    int32_t *end;           /* [E] end of the window the record was armed on                        */
    int32_t *ntx;           /* [E] transaction rows recorded                                        */
    int32_t *len;           /* [E] entries recorded                                                 */
    int32_t *flags;         /* [E] FINENV_HIST_ARMED / _COMPLETE / _OVERFLOW                        */
    int32_t  capacity;      /* >= 1                                                                 */
} finenv_twowave_history;
/* Attach a history (the struct is copied), or detach with NULL (the default).  Allowed before bind.
 * Attaching arms nothing: zero len / flags, then finenv_<kind>_reset / _history_arm. */
int finenv_cashpenalty_set_history(finenv_cashpenalty *h, const finenv_twowave_history *hist);
int finenv_stoploss_set_history(finenv_stoploss *h, const finenv_twowave_history *hist);
/* Arm every env, or those with mask[e] != 0 (device u8[E]), at its current date. */
int finenv_cashpenalty_history_arm(finenv_cashpenalty *h, const uint8_t *mask, void *stream);
int finenv_stoploss_history_arm(finenv_stoploss *h, const uint8_t *mask, void *stream);
/* Backtest figures of the recorded total assets cash + asset_value: out
 * [E][FINENV_STOCK_HISTORY_METRICS] f64, the FINENV_HM_* columns with the stock env's convention:
 * returns total[k] / total[k-1] - 1 in fp64 for k = 1 .. len-1, N_RETURNS = len - 1.  Rows of
 * unarmed envs and of empty records are NaN. */
int finenv_cashpenalty_history_metrics(finenv_cashpenalty *h, double annualization, double *out,
                                       void *stream);
int finenv_stoploss_history_metrics(finenv_stoploss *h, double annualization, double *out,
                                    void *stream);

/* =====================================================================================
 * BitcoinEnv (finrl/meta/env_cryptocurrency_trading/env_btc_ccxt.py:6-215), the single-asset
 * ElegantRL demo env.  NOT CryptoEnv with one asset: it may go short, buys fractional amounts, and
 * ADDS the discounted return to the terminal reward.
 *   actions [E][1] f32 (what ElegantRL's act(...).cpu().numpy()[0] hands over)
 *   obs     [E][D] f32, D = P + 9 = [account*2^-18 | price[day][0..P)*2^-15 |
 *           tech[day][0..7)*(2^-1, 2^-15, 2^-15, 2^-6, 2^-6, 2^-15, 2^-15) | stocks*2^-4] (:62-79)
 *   reward  (delta total asset) * 2^-16; on the last step PLUS the discounted return (:121-128)
 * Contract: price_ary [T][P] and tech_ary [T][W], W >= 7, are float64 and actions float32; every
 * other combination changes the reference's arithmetic under NumPy 2 (NEP 50) and is refused by
 * the Python layers.  Trades use price column 0.  With adj = price[day][0], a = action:
 *   a < 0   q = min(-a, (0.5 * total_asset) / adj + stocks) (ties keep -a), sold if q > 0 -- stocks may
 *           go NEGATIVE -- account += (adj * q) * (1 - fee); else account += (adj * 0) * (1 - fee) (:86-90)
 *   a > 0   q = min(a, account / adj), not clamped at 0; account -= (adj * q) * (1 + fee) (:92-95)
 *   then    day += 1; next = account + price[day][0] * stocks; reward = (next - total_asset) * 2^-16;
 *           gamma_return = gamma_return * gamma + reward; done = (day + 1 == rows); on done
 *           reward += gamma_return, gamma_return = 0, episode_return = next / initial_account
 * Every *, /, + is a float64 operation rounded on its own, in that order -- except `stocks`, whose
 * NumPy scalar type the reference's arithmetic depends on: a Python float after reset(), float32
 * after a trade of the action's own size, float64 once a cap has bound.  FINENV_BI_STOCKS_TAG keeps
 * it (FINENV_NT_PY / _F32 / _F64; a trade sets it to the larger of its own and the quantity's: F32
 * for the action, F64 for a cap), and while it is F32 `stocks +/- q` is a float32 operation.
 * reset() (:53-60) restores day, account, stocks (0.0, FINENV_NT_PY) and total_asset and, as in the
 * reference, leaves gamma_return and episode_return alone.
 * Defined here (the reference raises IndexError): an env stepped again on its terminal row --
 * after done, auto_reset off, no reset -- makes no trade and keeps its state; the step writes the
 * current observation, reward 0 (FINENV_BF_LAST_REWARD too) and done 1, and reads no row outside
 * the panel.
 *
 * Action and panel domain.  Prices are finite and > 0, at any magnitude (1e-4 .. 1e8 are tested), and
 * the initial account is any positive value (1e2 .. 1e12 are tested).  The reference divides by
 * price[day][0] unguarded (:87, :92): zero, negative, NaN and infinite prices are unspecified here --
 * no access outside the panel, no fault, values not defined.  Actions are ANY float32, and with prices
 * and account in the domain every state field, reward and observation stays finite:
 *   +-0, NaN      trade nothing (neither `a < 0` nor `a > 0` holds, :85, :91)
 *   |a| > 1       is not clipped; the two min()s are the only caps
 *   +-inf         always binds the cap (a sale is still dropped when the cap is <= 0)
 *   denormals     float32-denormal actions trade denormal amounts: while the tag is F32, `stocks +/- q`
 *                 keeps them (a float32 operation without flush to zero), and the observation's
 *                 stocks * 2^-4 is converted to a float32 denormal, not to 0
 * tests/test_gpu_btc_domain.py holds the kernel to this bit for bit, at the narrowest and the widest
 * row; tests/test_gpu_btc_launch_forms.py runs every launch form (D = 62 | 63, 126 | 127, 254).
 * ===================================================================================== */
#define FINENV_BTC_MAX_PRICE_COLS 245   /* D <= 254: a wave's observation rows fit one block's LDS */

typedef struct finenv_btc_config {
    int32_t n_envs;
    int32_t n_price_cols;         /* P = price_ary.shape[1] >= 1                         */
    int32_t n_tech_cols;          /* W = tech_ary.shape[1] >= 7 (the first 7 are shown)  */
    int32_t n_rows;               /* T = rows of the panel >= 2                          */
    int32_t reserved0;
    int32_t reserved1;
    double  initial_account;      /* :17                                                 */
    double  transaction_fee_percent;   /* :19                                            */
    double  gamma;                /* :21                                                 */
} finenv_btc_config;

typedef struct finenv_btc_panel {
    const double *price0;         /* [T] f64 = price_ary[:, 0], the traded column        */
    const float  *obs_tmpl;       /* [T][P + 7] f32: columns 1 .. D-2 of the observation row of each
                                     panel row, the reference's scaling expressions evaluated in
                                     float64 by the host and cast; the kernel copies them */
} finenv_btc_panel;

enum { FINENV_BF_ACCOUNT = 0, FINENV_BF_STOCKS, FINENV_BF_TOTAL_ASSET, FINENV_BF_GAMMA_RETURN,
       FINENV_BF_EPISODE_RETURN, FINENV_BF_LAST_REWARD, FINENV_BTC_F64_FIELDS };
enum { FINENV_BI_DAY = 0, FINENV_BI_STOCKS_TAG, FINENV_BTC_I32_FIELDS };
typedef struct finenv_btc_state {
    double  *f64;                 /* [FINENV_BTC_F64_FIELDS][E]; LAST_REWARD: the float64 reward of
                                     the last step (the reward output is its float32 cast) */
    int32_t *i32;                 /* [FINENV_BTC_I32_FIELDS][E]; DAY is the PANEL row     */
} finenv_btc_state;

typedef struct finenv_btc finenv_btc;

int  finenv_btc_create(const finenv_btc_config *cfg, finenv_btc **out);
void finenv_btc_destroy(finenv_btc *h);
const char *finenv_btc_last_error(const finenv_btc *h);
int  finenv_btc_obs_dim(const finenv_btc *h);
int  finenv_btc_bind(finenv_btc *h, const finenv_btc_panel *panel, const finenv_btc_state *state);
/* reset() (:53-79) of every env, or of those with mask[e] != 0; obs_out (may be NULL) receives the
 * rows of the envs it resets. */
int  finenv_btc_reset(finenv_btc *h, const uint8_t *mask, float *obs_out, void *stream);
/* step() (:81-129).  obs [E][D] f32 packed, reward [E] f32, done [E] u8; term_obs [E][D] or NULL:
 * rows of the envs that report done receive the observation the reference's last step() returns.
 * auto_reset: DummyVecEnv semantics inside the launch (a done env is reset and obs holds its first
 * observation).  The output pointers may address slice t of rollout tensors [n_steps][E][...]:
 * collecting a rollout needs no extra copy (any 4-byte aligned obs is taken; a 16-byte aligned one
 * is written faster). */
int  finenv_btc_step(finenv_btc *h, const float *actions, float *obs, float *reward, uint8_t *done,
                     float *term_obs, int32_t auto_reset, void *stream);

/* Per-env episode windows: many BitcoinEnv instances on row ranges of ONE bound panel in one batch
 * -- the train / test / trade modes of load_data (:176-215) side by side, or random training
 * windows.  The contract of finenv_stock_set_windows: caller-owned device block int32_t win[2][E],
 * win[0][e] = s_e (first panel row), win[1][e] = t_e (end, exclusive); env e then equals the
 * reference env whose arrays are rows [s_e, t_e): done when the incremented day equals t_e - 1, a
 * reset (host or auto) goes back to row s_e.  FINENV_BI_DAY stays the panel row (the reference's
 * self.day is FINENV_BI_DAY - s_e).  step() reads t_e on every step and s_e only when it resets an
 * env, so an edited end applies from the next step and an edited start at the env's next reset.
 * The kernels clamp both rows into the panel whatever the block holds: a bad window is a wrong
 * answer, never an access outside the panel; valid windows (0 <= s_e, s_e + 2 <= t_e <= n_rows) read
 * no row outside [s_e, t_e).  The pointer is a kernel argument: launches and graph replays see later
 * edits of the block's CONTENTS, a graph keeps the pointer it was captured with.  NULL detaches
 * (the default: every env runs rows 0 .. n_rows-1).  Works before bind.  Returns FINENV_ERR_INVALID
 * for a NULL handle. */
int  finenv_btc_set_windows(finenv_btc *h, int32_t *win);

/* =====================================================================================
 * Risk precompute that feeds the panels.  Stateless; all buffers are
 * caller-owned device memory; launches go to `stream`; nothing synchronises.
 * Floating point (tolerances in tests/test_gpu_riskpre_parity.py): covariance sums run in day
 * order (NumPy: BLAS), the pseudo-inverse is applied through a Jacobi eigen-decomposition
 * (NumPy: LAPACK SVD) with NumPy's cutoff 1e-15 * largest eigenvalue.
 * Contract: complete panel (every asset on every day, close > 0, no NaN).
 * ===================================================================================== */
#define FINENV_RISKPRE_MAX_ASSETS 128

/* DataFrame.pct_change() of the close pivot (preprocessors.py:219-221):
 * returns[t][j] = close[t][j] / close[t-1][j] - 1, row 0 = NaN.  close, returns: [T][N] f64 */
int finenv_riskpre_returns(const double *close, double *returns, int32_t n_days,
                           int32_t n_assets, void *stream);
/* FeatureEngineer.calculate_turbulence (preprocessors.py:215-267): turbulence[t] for all T days
 * (0 for t < window and for the first two positive values, :247-257).  quad: [T] f64 scratch
 * (the unfiltered quadratic forms, :244-246).  Needs n_days >= window (the reference raises
 * otherwise, :260-266) and 1 <= n_assets <= FINENV_RISKPRE_MAX_ASSETS (one asset: the 1 x 1
 * covariance, x^2 / var, or 0 where the window's variance is 0, as np.linalg.pinv gives). */
int finenv_riskpre_turbulence(const double *returns, double *quad, double *turbulence,
                              int32_t n_days, int32_t n_assets, int32_t window, void *stream);
/* cov_list of the portfolio-allocation tutorial
 * (tutorials/2-Advance/FinRL_PortfolioAllocation_Explainable_DRL.py:160-172): cov_out[i-lookback]
 * = sample covariance of the `lookback` returns ending at day i inclusive, for i in
 * [lookback, T).  cov_out: [T-lookback][N][N] f64. */
int finenv_riskpre_rolling_cov(const double *returns, double *cov_out, int32_t n_days,
                               int32_t n_assets, int32_t lookback, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FINENV_H */
