// finenv_stock_np128.hip -- step / aux kernels and launchers of the batched StockTradingEnv for
// 64 < N <= 128 tickers (NASDAQ-100): namespace np128, finenv_stock_impl::{choose_step,launch_aux}_np128.
#define FINENV_NP 128
#define FINENV_LOG2NP 7
#define FINENV_SORTNET "sortnet128.inc"
#include "finenv_stock_width.inc"
