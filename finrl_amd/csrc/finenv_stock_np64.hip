// finenv_stock_np64.hip -- step / aux kernels and launchers of the batched StockTradingEnv for
// 32 < N <= 64 tickers: namespace np64, finenv_stock_impl::{choose_step,launch_aux}_np64.
#define FINENV_NP 64
#define FINENV_LOG2NP 6
#define FINENV_SORTNET "sortnet64.inc"
#include "finenv_stock_width.inc"
