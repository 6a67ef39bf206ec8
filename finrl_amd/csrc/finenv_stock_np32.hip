// finenv_stock_np32.hip -- step / aux kernels and launchers of the batched StockTradingEnv for
// N <= 32 tickers (DOW30: the headline): namespace np32, finenv_stock_impl::{choose_step,launch_aux}_np32.
#define FINENV_NP 32
#define FINENV_LOG2NP 5
#define FINENV_SORTNET "sortnet32.inc"
#include "finenv_stock_width.inc"
