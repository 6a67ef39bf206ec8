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
STOCK_MAX_TICKERS = 128    # FINENV_STOCK_MAX_TICKERS
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


class VecNormPtrs(C.Structure):
    """finenv_vecnorm: a running-statistics block (mean / var / scale [dim], count), the partials
    buffer and ticket word of its update launch, dim, the partials capacity, epsilon and clip."""
    _fields_ = [("mean", C.c_void_p), ("var", C.c_void_p), ("scale", C.c_void_p), ("count", C.c_void_p),
                ("partials", C.c_void_p), ("ticket", C.c_void_p), ("dim", C.c_int32),
                ("partials_cap", C.c_int32), ("epsilon", C.c_double), ("clip", C.c_double)]


VECNORM_MAX_TILES = 128         # FINENV_VECNORM_MAX_TILES: 2 * this * dim doubles of partials always suffice


# Every struct of include/finenv.h: (C name, finenv_struct_size index, ctypes class).  The history structs
# have no index; 18, 22, 25, 27, 29 and 32 are no struct's (the library answers -1 there).
STRUCTS = (
    ("finenv_stock_config", 0, StockConfig),
    ("finenv_stock_panel", 1, StockPanelPtrs),
    ("finenv_stock_state", 2, StockStatePtrs),
    ("finenv_portfolio_config", 3, PortfolioConfig),
    ("finenv_portfolio_panel", 4, PortfolioPanelPtrs),
    ("finenv_portfolio_state", 5, PortfolioStatePtrs),
    ("finenv_crypto_config", 6, CryptoConfig),
    ("finenv_crypto_panel", 7, CryptoPanelPtrs),
    ("finenv_crypto_state", 8, CryptoStatePtrs),
    ("finenv_stocknp_config", 9, StockNpConfig),
    ("finenv_stocknp_panel", 10, StockNpPanelPtrs),
    ("finenv_stocknp_state", 11, StockNpStatePtrs),
    ("finenv_cashpenalty_config", 12, CashPenaltyConfig),
    ("finenv_cashpenalty_panel", 13, CashPenaltyPanelPtrs),
    ("finenv_cashpenalty_state", 14, CashPenaltyStatePtrs),
    ("finenv_stoploss_config", 15, StopLossConfig),
    ("finenv_stoploss_panel", 16, StopLossPanelPtrs),
    ("finenv_stoploss_state", 17, StopLossStatePtrs),
    ("finenv_btc_config", 19, BtcConfig),
    ("finenv_btc_panel", 20, BtcPanelPtrs),
    ("finenv_btc_state", 21, BtcStatePtrs),
    ("finenv_replay_view", 23, ReplayViewPtrs),
    ("finenv_replay_batch", 24, ReplayBatchPtrs),
    ("finenv_replay_nstep", 26, ReplayNStepPtrs),
    ("finenv_replay_per", 28, ReplayPerPtrs),
    ("finenv_rollout_view", 30, RolloutViewPtrs),
    ("finenv_rollout_batch", 31, RolloutBatchPtrs),
    ("finenv_vecnorm", 33, VecNormPtrs),
    ("finenv_stock_history", None, StockHistoryPtrs),
    ("finenv_portfolio_history", None, PortfolioHistoryPtrs),
    ("finenv_crypto_history", None, CryptoHistoryPtrs),
    ("finenv_stocknp_history", None, StockNpHistoryPtrs),
    ("finenv_twowave_history", None, TwoWaveHistoryPtrs),
)
V3_BASELINE_STRUCTS = 18        # indices 0 .. 17: what every ABI v3 build answers

# Every function of include/finenv.h: name -> (restype, argtypes).  A pointer to a struct above is
# POINTER(its class), `finenv_<kind> **` is POINTER(c_void_p), every other pointer (handles, device
# buffers, streams) is c_void_p; tests/test_native_abi.py holds each entry to its prototype.
INT, P, I32, I64, U64, F32, F64 = C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double
_view, _batch, _nstep, _per, _vn = (C.POINTER(s) for s in (
    ReplayViewPtrs, ReplayBatchPtrs, ReplayNStepPtrs, ReplayPerPtrs, VecNormPtrs))
_STEP = [P] * 6 + [I32, P]      # handle, actions, obs, reward, done, term_obs, auto_reset, stream

SIGNATURES = {
    "finenv_abi_version": (INT, []),
    "finenv_struct_size": (INT, [INT]),
    "finenv_strerror": (C.c_char_p, [INT]),
    "finenv_device_count": (INT, []),
    "finenv_stock_set_obs_pitch": (INT, [P, I32]),
    "finenv_stock_set_desync_hint": (INT, [P, I32]),
    "finenv_stock_init": (INT, [P, I32, P]),
    "finenv_stock_observe": (INT, [P] * 3),
    "finenv_stock_refresh": (INT, [P] * 2),
    "finenv_stock_step": (INT, [P] * 7 + [I32, P]),             # realised before auto_reset
    "finenv_stock_episode_stats": (INT, [P] * 3),
    "finenv_stock_set_last_episode": (INT, [P] * 2),
    "finenv_stock_last_episode_stats": (INT, [P] * 3),
    "finenv_portfolio_step": (INT, [P] * 7 + [I32, P]),         # weights_out before auto_reset
    "finenv_portfolio_set_last_episode": (INT, [P] * 2),
    "finenv_portfolio_last_episode_stats": (INT, [P] * 3),
    "finenv_crypto_step": (INT, _STEP),
    "finenv_crypto_step_record": (INT, [P] * 6 + [I32] + [P] * 6),
    "finenv_stocknp_set_obs_pitch": (INT, [P, I32]),
    "finenv_stocknp_step": (INT, _STEP),
    "finenv_cashpenalty_step": (INT, _STEP),
    "finenv_cashpenalty_set_random_start": (INT, [P, I32, U64]),
    "finenv_cashpenalty_set_audit": (INT, [P] * 2),
    "finenv_stoploss_step": (INT, _STEP),
    "finenv_stoploss_set_random_start": (INT, [P, I32, U64]),
    "finenv_stoploss_set_audit": (INT, [P] * 2),
    "finenv_btc_step": (INT, _STEP),
    "finenv_riskpre_returns": (INT, [P, P, I32, I32, P]),
    "finenv_riskpre_turbulence": (INT, [P, P, P, I32, I32, I32, P]),
    "finenv_riskpre_rolling_cov": (INT, [P, P, I32, I32, I32, P]),
    "finenv_gae_scan": (INT, [P] * 6 + [I32, I32, F32, F32, P]),
    "finenv_rollout_put": (INT, [P] * 6 + [I32, I32, P]),
    "finenv_rollout_minibatch": (INT, [C.POINTER(RolloutViewPtrs), P, U64, I64, C.POINTER(RolloutBatchPtrs),
                                       P, P]),
    "finenv_replay_put": (INT, [P, P, I32, P, I32, I32, P]),
    "finenv_replay_sample": (INT, [_view, P, P, U64, _batch, P, P]),
    "finenv_replay_gather": (INT, [_view, P, _batch, P]),
    "finenv_replay_sample_nstep": (INT, [_view, P, P, U64, _batch, _nstep, P, P]),
    "finenv_replay_gather_nstep": (INT, [_view, P, _batch, _nstep, P]),
    "finenv_replay_per_tree_words": (I64, [I64]),
    "finenv_replay_per_rebuild": (INT, [_per, I32, I32, P]),
    "finenv_replay_per_put": (INT, [_per, I32, I32, I32, I32, P]),
    "finenv_replay_per_update": (INT, [_per, I32, I32, P, P, I32, P]),
    "finenv_replay_per_find": (INT, [_per, I32, I32, P, I32, P, P]),
    "finenv_replay_per_sample": (INT, [_view, _per, P, U64, _batch, P, P, P]),
    "finenv_replay_per_sample_nstep": (INT, [_view, _per, P, U64, _batch, _nstep, P, P, P]),
    "finenv_vecnorm_refresh": (INT, [_vn, P]),
    "finenv_vecnorm_update": (INT, [_vn, P, I64, I64, P]),
    "finenv_vecnorm_apply": (INT, [_vn, P, I64, I64, P, I64, I32, P]),
    "finenv_vecnorm_step": (INT, [_vn, _vn, P, I64, P, P, P, F64, P, I64, P, P, I32, I32, I32, I32, P]),
}
# the entry points every kind has: (config, panel, state, history struct or None, set_windows pointers)
for _kind, (_cfg, _panel, _state, _hist, _win) in {
        "stock": (StockConfig, StockPanelPtrs, StockStatePtrs, StockHistoryPtrs, 1),
        "portfolio": (PortfolioConfig, PortfolioPanelPtrs, PortfolioStatePtrs, PortfolioHistoryPtrs, 1),
        "crypto": (CryptoConfig, CryptoPanelPtrs, CryptoStatePtrs, CryptoHistoryPtrs, 2),   # + norm_rows
        "stocknp": (StockNpConfig, StockNpPanelPtrs, StockNpStatePtrs, StockNpHistoryPtrs, 1),
        "cashpenalty": (CashPenaltyConfig, CashPenaltyPanelPtrs, CashPenaltyStatePtrs, TwoWaveHistoryPtrs, 1),
        "stoploss": (StopLossConfig, StopLossPanelPtrs, StopLossStatePtrs, TwoWaveHistoryPtrs, 1),
        "btc": (BtcConfig, BtcPanelPtrs, BtcStatePtrs, None, 1)}.items():
    SIGNATURES.update({
        f"finenv_{_kind}_create": (INT, [C.POINTER(_cfg), C.POINTER(P)]),
        f"finenv_{_kind}_destroy": (None, [P]),
        f"finenv_{_kind}_last_error": (C.c_char_p, [P]),
        f"finenv_{_kind}_obs_dim": (INT, [P]),
        f"finenv_{_kind}_bind": (INT, [P, C.POINTER(_panel), C.POINTER(_state)]),
        f"finenv_{_kind}_reset": (INT, [P] * 4),
        f"finenv_{_kind}_set_windows": (INT, [P] * (1 + _win)),
    })
    if _hist is not None:
        SIGNATURES.update({
            f"finenv_{_kind}_set_history": (INT, [P, C.POINTER(_hist)]),
            f"finenv_{_kind}_history_arm": (INT, [P] * 3),
            f"finenv_{_kind}_history_metrics": (INT, [P, F64, P, P]),
        })


def declare(L):
    """Declare the tables on a loaded library and check it against them.  One rule lets a build of an
    earlier commit load beside the current one (tools/exp_ab_inproc.py): a function the library does not
    export is not declared, and past the v3 baseline a struct index it answers -1 for is one it predates.
    Any other size than the class's, or -1 inside the baseline, raises."""
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    if L.finenv_abi_version() != ABI_VERSION:
        raise NativeLibraryError("libfinenv.so ABI version mismatch; rebuild (make -C finrl_amd/csrc)")
    for _, which, cls in STRUCTS:
        if which is None:
            continue
        size = L.finenv_struct_size(which)
        if size != C.sizeof(cls) and not (size == -1 and which >= V3_BASELINE_STRUCTS):
            raise NativeLibraryError(
                f"ABI struct size mismatch for {cls.__name__}: python {C.sizeof(cls)} vs library {size}")
    return L


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
    _lib = declare(C.CDLL(LIB_PATH))
    return _lib


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
