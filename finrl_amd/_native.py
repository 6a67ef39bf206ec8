"""ctypes binding of libfinenv.so (include/finenv.h).  Fails loudly: no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# FINENV_LIB overrides the library path (diagnostic builds, e.g. libfinenv_diag.so)
LIB_PATH = os.environ.get("FINENV_LIB") or os.path.join(_HERE, "lib", "libfinenv.so")
CSRC_DIR = os.path.join(_HERE, "csrc")

FINENV_OK = 0
ABI_VERSION = 3            # include/finenv.h FINENV_ABI_VERSION
AUDIT_HEAD = 4             # FINENV_AUDIT_HEAD: begin cash, asset value, reward, flags
AUDIT_F_LAST_DATE, AUDIT_F_CASH_SHORTAGE, AUDIT_F_TURBULENCE, AUDIT_F_STOP_LOSS, \
    AUDIT_F_LOW_PROFIT, AUDIT_F_HIGH_PROFIT = 1, 2, 4, 8, 16, 32


class NativeLibraryError(ImportError):
    pass


class FinenvError(RuntimeError):
    pass


def build(force: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", CSRC_DIR, "-s"] + (["-B"] if force else [])
    subprocess.check_call(args)
    return LIB_PATH


class StockConfig(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32), ("n_tickers", C.c_int32), ("n_tech", C.c_int32),
        ("n_days", C.c_int32), ("hmax", C.c_int32), ("use_turbulence", C.c_int32),
        ("reset_quirk", C.c_int32), ("initial", C.c_int32), ("track_stats", C.c_int32),
        ("single_ticker", C.c_int32),
        ("buy_cost_pct", C.c_double), ("sell_cost_pct", C.c_double),
        ("reward_scaling", C.c_double), ("turbulence_threshold", C.c_double),
    ]


class StockPanelPtrs(C.Structure):
    _fields_ = [("close", C.c_void_p), ("obs_tmpl", C.c_void_p), ("risk", C.c_void_p)]


# Field order of the two [field][E] state blocks (include/finenv.h enums)
STOCK_F64_FIELDS = ("cash", "cost", "last_reward", "turbulence", "asset0", "ret_sum", "ret_sumsq",
                    "cash0", "begin_asset")
STOCK_I32_FIELDS = ("day", "price_day", "trades", "episode", "start_day")
# Field order of the last-episode block (FINENV_SL_*): f64 [field][E]
STOCK_LAST_FIELDS = ("count", "episode", "begin_asset", "end_asset", "cost", "trades", "ret_n",
                     "ret_sum", "ret_sumsq")


class StockStatePtrs(C.Structure):
    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p)]


class StockHistoryPtrs(C.Structure):
    """finenv_stock_history: the episode-history tensors of finenv_stock_set_history."""
    _fields_ = [("asset", C.c_void_p), ("row", C.c_void_p), ("actions", C.c_void_p),
                ("len", C.c_void_p), ("flags", C.c_void_p), ("capacity", C.c_int32)]


HIST_COMPLETE, HIST_OVERFLOW = 1, 2          # FINENV_HIST_*: bits of the history's flags
HIST_ARMED = 4                               # (the cash-penalty / stop-loss record: len 0 is an armed record)
# columns of finenv_stock_history_metrics (FINENV_HM_*)
STOCK_HISTORY_METRICS = ("n_returns", "cumulative_return", "mean", "std", "sharpe", "max_drawdown")


class PortfolioConfig(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("n_tickers", C.c_int32), ("n_tech", C.c_int32),
                ("n_days", C.c_int32), ("initial_amount", C.c_double)]


class PortfolioPanelPtrs(C.Structure):
    _fields_ = [("gross_ret", C.c_void_p), ("obs_tmpl", C.c_void_p)]


PORTFOLIO_F64_FIELDS = ("value", "last_reward")
PORTFOLIO_I32_FIELDS = ("day",)
# Field order of the portfolio env's last-episode block (FINENV_PL_*): f64 [field][E]
PORTFOLIO_LAST_FIELDS = ("count", "begin_value", "end_value", "ret_n", "ret_sum", "ret_sumsq",
                         "run_sum", "run_sumsq")


class PortfolioStatePtrs(C.Structure):
    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p)]


class PortfolioHistoryPtrs(C.Structure):
    """finenv_portfolio_history: the episode-history tensors of finenv_portfolio_set_history."""
    _fields_ = [("value", C.c_void_p), ("ret", C.c_void_p), ("row", C.c_void_p),
                ("weights", C.c_void_p), ("len", C.c_void_p), ("flags", C.c_void_p),
                ("capacity", C.c_int32)]


# columns of finenv_portfolio_history_metrics: the FINENV_HM_* indices (n_returns counts the leading 0)
PORTFOLIO_HISTORY_METRICS = STOCK_HISTORY_METRICS


class CryptoConfig(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("n_assets", C.c_int32), ("n_tech", C.c_int32),
                ("n_steps", C.c_int32), ("lookback", C.c_int32), ("reserved0", C.c_int32),
                ("initial_cash", C.c_double), ("buy_cost_pct", C.c_double),
                ("sell_cost_pct", C.c_double), ("gamma", C.c_double)]


class CryptoPanelPtrs(C.Structure):
    _fields_ = [("price", C.c_void_p), ("tech_scaled", C.c_void_p), ("norm", C.c_void_p)]


CRYPTO_F64_FIELDS = ("cash", "total_asset", "gamma_return", "episode_return", "last_reward")
CRYPTO_I32_FIELDS = ("time",)


class CryptoStatePtrs(C.Structure):
    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p), ("stocks", C.c_void_p)]


class CryptoHistoryPtrs(C.Structure):
    """finenv_crypto_history: the episode-history tensors of finenv_crypto_set_history."""
    _fields_ = [("asset", C.c_void_p), ("holdings", C.c_void_p), ("stocks", C.c_void_p),
                ("start", C.c_void_p), ("len", C.c_void_p), ("flags", C.c_void_p),
                ("capacity", C.c_int32)]


# columns of finenv_crypto_history_metrics: the FINENV_HM_* indices, n_returns = len - 1 as in the stock env
CRYPTO_HISTORY_METRICS = STOCK_HISTORY_METRICS


class StockNpConfig(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("n_tickers", C.c_int32), ("n_techw", C.c_int32),
                ("n_days", C.c_int32), ("min_action", C.c_int32), ("reserved0", C.c_int32),
                ("max_stock", C.c_double), ("buy_cost_pct", C.c_double),
                ("sell_cost_pct", C.c_double), ("reward_scaling", C.c_double),
                ("gamma", C.c_double), ("obs_amount_floor", C.c_double)]


class StockNpPanelPtrs(C.Structure):
    _fields_ = [("price", C.c_void_p), ("obs_tmpl", C.c_void_p), ("turb_bool", C.c_void_p)]


STOCKNP_F64_FIELDS = ("amount", "total_asset", "gamma_reward", "initial_total_asset",
                      "episode_return", "last_reward", "amount0")
STOCKNP_I32_FIELDS = ("day", "tags", "amount0_tag")


class StockNpStatePtrs(C.Structure):
    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p), ("f32", C.c_void_p)]


class StockNpHistoryPtrs(C.Structure):
    """finenv_stocknp_history: the episode-history tensors of finenv_stocknp_set_history."""
    _fields_ = [("asset", C.c_void_p), ("tag", C.c_void_p), ("stocks", C.c_void_p),
                ("start", C.c_void_p), ("len", C.c_void_p), ("flags", C.c_void_p),
                ("capacity", C.c_int32)]


# columns of finenv_stocknp_history_metrics: the FINENV_HM_* indices, n_returns = len - 1 as in the stock env
STOCKNP_HISTORY_METRICS = STOCK_HISTORY_METRICS


class CashPenaltyConfig(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("n_assets", C.c_int32), ("n_cols", C.c_int32),
                ("n_days", C.c_int32), ("discrete_actions", C.c_int32),
                ("shares_increment", C.c_int32), ("use_turbulence", C.c_int32),
                ("patient", C.c_int32), ("hmax", C.c_double), ("buy_cost_pct", C.c_double),
                ("sell_cost_pct", C.c_double), ("initial_amount", C.c_double),
                ("cash_penalty_proportion", C.c_double), ("turbulence_threshold", C.c_double)]


class CashPenaltyPanelPtrs(C.Structure):
    _fields_ = [("close", C.c_void_p), ("info", C.c_void_p), ("turb", C.c_void_p)]


CASHPENALTY_F64_FIELDS = ("coh", "turbulence", "sum_trades", "logged_total", "logged_cash")
CASHPENALTY_I32_FIELDS = ("date_index", "start", "episode", "next_start")


class CashPenaltyStatePtrs(C.Structure):
    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p)]


class StopLossConfig(C.Structure):
    _fields_ = CashPenaltyConfig._fields_ + [("stoploss_penalty", C.c_double),
                                             ("min_profit_penalty", C.c_double)]


class StopLossPanelPtrs(C.Structure):
    _fields_ = [("close", C.c_void_p), ("info", C.c_void_p), ("turb", C.c_void_p)]


STOPLOSS_F64_FIELDS = ("coh", "turbulence", "sum_trades", "logged_total", "logged_cash",
                       "actual_num_trades")
STOPLOSS_BOOKS = ("holdings", "prev_holdings", "closing_diff_avg_buy",
                  "profit_sell_diff_avg_buy", "n_buys", "avg_buy_price")
STOPLOSS_I32_FIELDS = ("date_index", "start", "episode", "next_start")


class StopLossStatePtrs(C.Structure):
    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p)]


class TwoWaveHistoryPtrs(C.Structure):
    """finenv_twowave_history: the episode-history tensors of finenv_{cashpenalty,stoploss}_set_history."""
    _fields_ = [("cash", C.c_void_p), ("asset_value", C.c_void_p), ("reward", C.c_void_p),
                ("reason", C.c_void_p), ("transactions", C.c_void_p), ("actions", C.c_void_p),
                ("start", C.c_void_p), ("end", C.c_void_p), ("ntx", C.c_void_p),
                ("len", C.c_void_p), ("flags", C.c_void_p), ("capacity", C.c_int32)]


# columns of finenv_{cashpenalty,stoploss}_history_metrics: the FINENV_HM_* indices over cash + asset_value,
# n_returns = len - 1 as in the stock env
TWOWAVE_HISTORY_METRICS = STOCK_HISTORY_METRICS


class BtcConfig(C.Structure):
    _fields_ = [("n_envs", C.c_int32), ("n_price_cols", C.c_int32), ("n_tech_cols", C.c_int32),
                ("n_rows", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32),
                ("initial_account", C.c_double), ("transaction_fee_percent", C.c_double),
                ("gamma", C.c_double)]


class BtcPanelPtrs(C.Structure):
    _fields_ = [("price0", C.c_void_p), ("obs_tmpl", C.c_void_p)]


BTC_F64_FIELDS = ("account", "stocks", "total_asset", "gamma_return", "episode_return", "last_reward")
BTC_I32_FIELDS = ("day", "stocks_tag")
BTC_MAX_PRICE_COLS = 245   # FINENV_BTC_MAX_PRICE_COLS


class BtcStatePtrs(C.Structure):
    _fields_ = [("f64", C.c_void_p), ("i32", C.c_void_p)]


# finenv_struct_size indices of the struct trios added after the first v3 list (0 .. 17 are the six
# kinds of lib()'s table in order; 18 stays invalid)
_LATER_STRUCTS = {19: BtcConfig, 20: BtcPanelPtrs, 21: BtcStatePtrs}


class ReplayViewPtrs(C.Structure):
    """finenv_replay_view: the four ring tensors of a replay buffer and S, E, D, P, A."""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("rewards", C.c_void_p),
                ("dones", C.c_void_p), ("n_slots", C.c_int32), ("n_envs", C.c_int32),
                ("obs_dim", C.c_int32), ("obs_pitch", C.c_int32), ("action_dim", C.c_int32),
                ("reserved0", C.c_int32)]


class ReplayBatchPtrs(C.Structure):
    """finenv_replay_batch: the five outputs of a sampled batch, B and the observation row pitch."""
    _fields_ = [("observations", C.c_void_p), ("next_observations", C.c_void_p),
                ("actions", C.c_void_p), ("rewards", C.c_void_p), ("dones", C.c_void_p),
                ("batch_size", C.c_int32), ("obs_pitch", C.c_int32)]


class ReplayNStepPtrs(C.Structure):
    """finenv_replay_nstep: the head words, the discount / steps outputs, n_steps and gamma."""
    _fields_ = [("head", C.c_void_p), ("discounts", C.c_void_p), ("steps", C.c_void_p),
                ("n_steps", C.c_int32), ("gamma", C.c_float)]


class ReplayPerPtrs(C.Structure):
    """finenv_replay_per: the tickets, the sum tree, the largest-ticket word and frac_bits."""
    _fields_ = [("tickets", C.c_void_p), ("tree", C.c_void_p), ("max_ticket", C.c_void_p),
                ("frac_bits", C.c_int32), ("reserved0", C.c_int32)]


# the replay buffer's pointer structs (22 stays invalid, like 18)
_REPLAY_STRUCTS = {23: ReplayViewPtrs, 24: ReplayBatchPtrs}
# the n-step sampler's (25 stays invalid: the end of the list above)
_REPLAY_NSTEP_STRUCTS = {26: ReplayNStepPtrs}
# prioritised replay's (27 stays invalid: the end of the list above)
_REPLAY_PER_STRUCTS = {28: ReplayPerPtrs}


class RolloutViewPtrs(C.Structure):
    """finenv_rollout_view: the six rollout tensors a minibatch reads and n_steps, E, D, P, A."""
    _fields_ = [("obs", C.c_void_p), ("actions", C.c_void_p), ("values", C.c_void_p),
                ("log_probs", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
                ("n_steps", C.c_int32), ("n_envs", C.c_int32), ("obs_dim", C.c_int32),
                ("obs_pitch", C.c_int32), ("action_dim", C.c_int32), ("reserved0", C.c_int32)]


class RolloutBatchPtrs(C.Structure):
    """finenv_rollout_batch: the six outputs of a minibatch, B and the observation row pitch."""
    _fields_ = [("observations", C.c_void_p), ("actions", C.c_void_p), ("old_values", C.c_void_p),
                ("old_log_prob", C.c_void_p), ("advantages", C.c_void_p), ("returns", C.c_void_p),
                ("batch_size", C.c_int32), ("obs_pitch", C.c_int32)]


# the rollout minibatch's (29 stays invalid: the end of the list above)
_ROLLOUT_STRUCTS = {30: RolloutViewPtrs, 31: RolloutBatchPtrs}


class VecNormPtrs(C.Structure):
    """finenv_vecnorm: a running-statistics block (mean / var / scale [dim], count), the partials
    buffer and ticket word of its update launch, dim, the partials capacity, epsilon and clip."""
    _fields_ = [("mean", C.c_void_p), ("var", C.c_void_p), ("scale", C.c_void_p), ("count", C.c_void_p),
                ("partials", C.c_void_p), ("ticket", C.c_void_p), ("dim", C.c_int32),
                ("partials_cap", C.c_int32), ("epsilon", C.c_double), ("clip", C.c_double)]


VECNORM_MAX_TILES = 128         # FINENV_VECNORM_MAX_TILES: 2 * this * dim doubles of partials always suffice
# the running statistics' (32 stays invalid: the end of the list above)
_VECNORM_STRUCTS = {33: VecNormPtrs}

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C finrl_amd/csrc` (needs hipcc). finrl_amd has no CPU "
            "fallback.")
    L = C.CDLL(LIB_PATH)
    L.finenv_abi_version.restype = C.c_int
    L.finenv_strerror.restype = C.c_char_p
    L.finenv_strerror.argtypes = [C.c_int]
    L.finenv_device_count.restype = C.c_int
    # entry points every kind has; each *_step is declared below (their signatures differ)
    for kind, cfg, panel, state in (
            ("stock", StockConfig, StockPanelPtrs, StockStatePtrs),
            ("portfolio", PortfolioConfig, PortfolioPanelPtrs, PortfolioStatePtrs),
            ("crypto", CryptoConfig, CryptoPanelPtrs, CryptoStatePtrs),
            ("stocknp", StockNpConfig, StockNpPanelPtrs, StockNpStatePtrs),
            ("cashpenalty", CashPenaltyConfig, CashPenaltyPanelPtrs, CashPenaltyStatePtrs),
            ("stoploss", StopLossConfig, StopLossPanelPtrs, StopLossStatePtrs),
            ("btc", BtcConfig, BtcPanelPtrs, BtcStatePtrs)):
        if kind == "btc" and not hasattr(L, "finenv_btc_create"):
            continue            # (a build of an earlier commit: see the note on the windows below)
        create, destroy, last_error, obs_dim, bind, reset = (
            getattr(L, f"finenv_{kind}_{name}")
            for name in ("create", "destroy", "last_error", "obs_dim", "bind", "reset"))
        create.argtypes = [C.POINTER(cfg), C.POINTER(C.c_void_p)]
        destroy.argtypes = [C.c_void_p]
        destroy.restype = None
        last_error.argtypes = [C.c_void_p]
        last_error.restype = C.c_char_p
        obs_dim.argtypes = [C.c_void_p]
        bind.argtypes = [C.c_void_p, C.POINTER(panel), C.POINTER(state)]
        reset.argtypes = [C.c_void_p] * 4
    L.finenv_stock_set_obs_pitch.argtypes = [C.c_void_p, C.c_int32]
    L.finenv_stock_set_desync_hint.argtypes = [C.c_void_p, C.c_int32]
    L.finenv_stock_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.finenv_stock_observe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.finenv_stock_refresh.argtypes = [C.c_void_p, C.c_void_p]
    L.finenv_stock_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.finenv_stock_episode_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.finenv_portfolio_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_void_p]
    L.finenv_crypto_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_void_p]
    L.finenv_crypto_step_record.argtypes = [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 6
    L.finenv_stocknp_set_obs_pitch.argtypes = [C.c_void_p, C.c_int32]
    L.finenv_stocknp_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int32, C.c_void_p]
    L.finenv_cashpenalty_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.finenv_stoploss_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(L, "finenv_btc_create"):
        L.finenv_btc_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int32, C.c_void_p]
        L.finenv_btc_set_windows.argtypes = [C.c_void_p] * 2
    L.finenv_riskpre_returns.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.finenv_riskpre_turbulence.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_void_p]
    L.finenv_riskpre_rolling_cov.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_void_p]
    L.finenv_cashpenalty_set_random_start.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
    L.finenv_stoploss_set_random_start.argtypes = [C.c_void_p, C.c_int32, C.c_uint64]
    L.finenv_cashpenalty_set_audit.argtypes = [C.c_void_p, C.c_void_p]
    L.finenv_stoploss_set_audit.argtypes = [C.c_void_p, C.c_void_p]
    # Last-episode block, episode windows.  Bound only where exported: tools/exp_ab_inproc.py loads a build of an
    # earlier commit through this function beside the current one (tests/test_native_abi.py checks
    # that the current build exports every symbol the header declares).
    for name, n in (("finenv_stock_set_last_episode", 2), ("finenv_stock_last_episode_stats", 3),
                    ("finenv_portfolio_set_last_episode", 2),
                    ("finenv_portfolio_last_episode_stats", 3), ("finenv_stock_set_windows", 2),
                    ("finenv_portfolio_set_windows", 2), ("finenv_crypto_set_windows", 3),
                    ("finenv_stocknp_set_windows", 2), ("finenv_cashpenalty_set_windows", 2),
                    ("finenv_stoploss_set_windows", 2)):
        if hasattr(L, name):
            getattr(L, name).argtypes = [C.c_void_p] * n
    for kind, ptrs in (("stock", StockHistoryPtrs), ("portfolio", PortfolioHistoryPtrs),
                       ("crypto", CryptoHistoryPtrs), ("stocknp", StockNpHistoryPtrs),
                       ("cashpenalty", TwoWaveHistoryPtrs), ("stoploss", TwoWaveHistoryPtrs)):
        if hasattr(L, f"finenv_{kind}_set_history"):       # episode history (same rule)
            getattr(L, f"finenv_{kind}_set_history").argtypes = [C.c_void_p, C.POINTER(ptrs)]
            getattr(L, f"finenv_{kind}_history_arm").argtypes = [C.c_void_p] * 3
            getattr(L, f"finenv_{kind}_history_metrics").argtypes = [C.c_void_p, C.c_double,
                                                                     C.c_void_p, C.c_void_p]
    if hasattr(L, "finenv_replay_put"):                    # replay buffer (same rule)
        L.finenv_replay_put.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_void_p]
        L.finenv_replay_sample.argtypes = [C.POINTER(ReplayViewPtrs), C.c_void_p, C.c_void_p,
                                           C.c_uint64, C.POINTER(ReplayBatchPtrs), C.c_void_p,
                                           C.c_void_p]
        L.finenv_replay_gather.argtypes = [C.POINTER(ReplayViewPtrs), C.c_void_p,
                                           C.POINTER(ReplayBatchPtrs), C.c_void_p]
    if hasattr(L, "finenv_replay_sample_nstep"):           # n-step sampler (same rule)
        L.finenv_replay_sample_nstep.argtypes = [
            C.POINTER(ReplayViewPtrs), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(ReplayBatchPtrs),
            C.POINTER(ReplayNStepPtrs), C.c_void_p, C.c_void_p]
        L.finenv_replay_gather_nstep.argtypes = [
            C.POINTER(ReplayViewPtrs), C.c_void_p, C.POINTER(ReplayBatchPtrs),
            C.POINTER(ReplayNStepPtrs), C.c_void_p]
    if hasattr(L, "finenv_replay_per_sample"):             # prioritised replay (same rule)
        per = C.POINTER(ReplayPerPtrs)
        L.finenv_replay_per_tree_words.argtypes = [C.c_int64]
        L.finenv_replay_per_tree_words.restype = C.c_int64
        L.finenv_replay_per_rebuild.argtypes = [per, C.c_int32, C.c_int32, C.c_void_p]
        L.finenv_replay_per_put.argtypes = [per, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_void_p]
        L.finenv_replay_per_update.argtypes = [per, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_int32, C.c_void_p]
        L.finenv_replay_per_find.argtypes = [per, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                             C.c_void_p, C.c_void_p]
        L.finenv_replay_per_sample.argtypes = [
            C.POINTER(ReplayViewPtrs), per, C.c_void_p, C.c_uint64, C.POINTER(ReplayBatchPtrs),
            C.c_void_p, C.c_void_p, C.c_void_p]
        L.finenv_replay_per_sample_nstep.argtypes = [
            C.POINTER(ReplayViewPtrs), per, C.c_void_p, C.c_uint64, C.POINTER(ReplayBatchPtrs),
            C.POINTER(ReplayNStepPtrs), C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "finenv_rollout_minibatch"):             # shuffled rollout minibatches (same rule)
        L.finenv_rollout_minibatch.argtypes = [
            C.POINTER(RolloutViewPtrs), C.c_void_p, C.c_uint64, C.c_int64, C.POINTER(RolloutBatchPtrs),
            C.c_void_p, C.c_void_p]
    if hasattr(L, "finenv_vecnorm_step"):                  # running obs / return statistics (same rule)
        vn = C.POINTER(VecNormPtrs)
        L.finenv_vecnorm_refresh.argtypes = [vn, C.c_void_p]
        L.finenv_vecnorm_update.argtypes = [vn, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        L.finenv_vecnorm_apply.argtypes = [vn, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                           C.c_int32, C.c_void_p]
        L.finenv_vecnorm_step.argtypes = [
            vn, vn, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p,
            C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    if L.finenv_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libfinenv.so ABI version mismatch; rebuild (make -C finrl_amd/csrc)")
    L.finenv_struct_size.argtypes = [C.c_int]
    first = (StockConfig, StockPanelPtrs, StockStatePtrs, PortfolioConfig, PortfolioPanelPtrs,
             PortfolioStatePtrs, CryptoConfig, CryptoPanelPtrs, CryptoStatePtrs, StockNpConfig,
             StockNpPanelPtrs, StockNpStatePtrs, CashPenaltyConfig, CashPenaltyPanelPtrs,
             CashPenaltyStatePtrs, StopLossConfig, StopLossPanelPtrs, StopLossStatePtrs)
    later = sorted(_LATER_STRUCTS.items()) if hasattr(L, "finenv_btc_create") else []
    if hasattr(L, "finenv_replay_put"):
        later += sorted(_REPLAY_STRUCTS.items())
    if hasattr(L, "finenv_replay_sample_nstep"):
        later += sorted(_REPLAY_NSTEP_STRUCTS.items())
    if hasattr(L, "finenv_replay_per_sample"):
        later += sorted(_REPLAY_PER_STRUCTS.items())
    if hasattr(L, "finenv_rollout_minibatch"):
        later += sorted(_ROLLOUT_STRUCTS.items())
    if hasattr(L, "finenv_vecnorm_step"):
        later += sorted(_VECNORM_STRUCTS.items())
    for which, cls in list(enumerate(first)) + later:
        if L.finenv_struct_size(which) != C.sizeof(cls):
            raise NativeLibraryError(
                f"ABI struct size mismatch for {cls.__name__}: python {C.sizeof(cls)} vs "
                f"library {L.finenv_struct_size(which)}")
    _lib = L
    return L


def check(code: int, handle=None, what: str = "", kind: str = "stock"):
    if code == FINENV_OK:
        return
    L = lib()
    msg = L.finenv_strerror(code).decode()
    if handle:
        detail = getattr(L, f"finenv_{kind}_last_error")(handle).decode()
        if detail:
            msg = f"{msg}: {detail}"
    raise FinenvError(f"{what or 'finenv'} failed ({code}): {msg}")
