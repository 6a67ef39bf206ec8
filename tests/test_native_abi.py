"""CPU-side checks of the C-ABI library: it loads (hipcc-built, no GPU needed), exports every
symbol include/finenv.h declares, the ctypes struct layouts match the compiled ones, argument
validation works, and launches fail loudly (never fall back) when no HIP device exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def test_exports_every_declared_symbol(L):
    hdr = open(os.path.join(ROOT, "include", "finenv.h")).read()
    names = sorted(set(re.findall(r"\b(finenv_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) >= 13
    for n in names:
        assert hasattr(L, n), f"libfinenv.so does not export {n}"


def test_struct_layouts_match(L):
    from finrl_amd import _native as nat
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    assert L.finenv_struct_size(0) == C.sizeof(nat.StockConfig)
    assert L.finenv_struct_size(1) == C.sizeof(nat.StockPanelPtrs)
    assert L.finenv_struct_size(2) == C.sizeof(nat.StockStatePtrs)
    hdr = open(os.path.join(ROOT, "include", "finenv.h")).read()
    f64 = re.findall(r"^\s+FINENV_SF_([A-Z0-9_]+)", hdr, flags=re.M)
    i32 = re.findall(r"^\s+FINENV_SI_([A-Z0-9_]+)", hdr, flags=re.M)
    assert tuple(x.lower() for x in f64) == nat.STOCK_F64_FIELDS
    assert tuple(x.lower() for x in i32) == nat.STOCK_I32_FIELDS


def test_create_validates_arguments(L):
    from finrl_amd import _native as nat
    h = C.c_void_p()
    ok = nat.StockConfig(64, 30, 8, 100, 100, 0, 1, 1, 1, 0, 1e-3, 1e-3, 1e-4, 0.0)
    assert L.finenv_stock_create(C.byref(ok), C.byref(h)) == 0
    assert L.finenv_stock_obs_dim(h) == 301
    # stepping before bind must fail with UNBOUND, not crash
    assert L.finenv_stock_step(h, None, None, None, None, None, None, 1, None) == -2
    assert b"bind" in L.finenv_stock_last_error(h)
    L.finenv_stock_destroy(h)
    for bad in (dict(n_tickers=129), dict(n_tickers=0), dict(n_envs=0), dict(n_days=0),
                dict(hmax=-1), dict(n_envs=2**30)):
        cfg = nat.StockConfig(64, 30, 8, 100, 100, 0, 1, 1, 1, 0, 1e-3, 1e-3, 1e-4, 0.0)
        for k, v in bad.items():
            setattr(cfg, k, v)
        assert L.finenv_stock_create(C.byref(cfg), C.byref(h)) == -1, bad
    assert L.finenv_strerror(-3) == b"HIP runtime error"


def test_no_cpu_fallback():
    """Without a HIP device the product must refuse to run, not quietly compute on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from finrl_amd import StockPanel
    from finrl_amd import _native as nat
    from finrl_amd.vec_env import VecStockTradingEnv
    panel = StockPanel(np.ones((4, 3)), np.zeros((4, 2, 3)), np.zeros(4))
    with pytest.raises((nat.FinenvError, RuntimeError, AssertionError)):
        VecStockTradingEnv(panel, 8, device="cpu")
    with pytest.raises(Exception):
        VecStockTradingEnv(panel, 8, device="cuda")
    assert nat.lib().finenv_device_count() <= 0


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under finrl_amd/ (the product) or tools/ (measurement
    helpers) may import or load it -- only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline legs."""
    for top in ("finrl_amd", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith((".py", ".hip", ".h", ".cpp", ".sh")):
                    txt = open(os.path.join(dirpath, f)).read()
                    assert "import oracle" not in txt and "from oracle" not in txt and \
                        "liboracle" not in txt, os.path.join(dirpath, f)
    bench = open(os.path.join(ROOT, "bench.py")).read()
    for line in bench.splitlines():          # every oracle import of bench.py sits in a cpu_baseline leg
        if "from oracle" in line or "import oracle" in line:
            assert line.startswith("    "), line


# One valid config per handle kind, the obs_dim it gives, and the entry points that launch work
# (name, argument count after the handle).  The host contract below holds for every kind alike.
def _kind_cases():
    from finrl_amd import _native as nat
    cash = (64, 4, 3, 50, 0, 1, 0, 0, 10.0, 3e-3, 3e-3, 1e6, 0.1, 0.0)
    return {
        "stock": (nat.StockConfig(64, 30, 8, 100, 100, 0, 1, 1, 1, 0, 1e-3, 1e-3, 1e-4, 0.0),
                  nat.StockPanelPtrs, 301,
                  (("init", 2), ("reset", 3), ("observe", 2), ("refresh", 1), ("step", 8),
                   ("episode_stats", 2), ("last_episode_stats", 2))),
        "portfolio": (nat.PortfolioConfig(64, 5, 4, 50, 1e6), nat.PortfolioPanelPtrs, 45,
                      (("reset", 3), ("step", 8), ("last_episode_stats", 2))),
        "crypto": (nat.CryptoConfig(64, 3, 4, 50, 2, 0, 1e6, 1e-3, 1e-3, 0.99),
                   nat.CryptoPanelPtrs, 12, (("reset", 3), ("step", 7), ("step_record", 12))),
        "stocknp": (nat.StockNpConfig(64, 5, 7, 50, 10, 0, 100.0, 1e-3, 1e-3, 2 ** -11, 0.99, 0.0),
                    nat.StockNpPanelPtrs, 25, (("reset", 3), ("step", 7))),
        "cashpenalty": (nat.CashPenaltyConfig(*cash), nat.CashPenaltyPanelPtrs, 17,
                        (("reset", 3), ("step", 7))),
        "stoploss": (nat.StopLossConfig(*cash, 0.9, 1.2), nat.StopLossPanelPtrs, 17,
                     (("reset", 3), ("step", 7))),
    }


@pytest.mark.parametrize("kind", ["stock", "portfolio", "crypto", "stocknp", "cashpenalty", "stoploss"])
def test_host_contract_every_kind(L, kind):
    """Null handles, create / obs_dim, launches before bind and bind with a null state pointer give
    the same codes and messages in every env's C ABI (no GPU needed: nothing here launches)."""
    cfg, panel_cls, D, launches = _kind_cases()[kind]
    fn = lambda name: getattr(L, f"finenv_{kind}_{name}")          # noqa: E731

    def launch(name, h):        # a private function object: the library's own argtypes stay as declared
        f = L[f"finenv_{kind}_{name}"]
        nargs = dict(launches)[name]
        f.argtypes = [C.c_void_p] * (1 + nargs)
        return f(h, *([None] * nargs))

    assert fn("last_error")(None) == b"null handle"
    assert fn("obs_dim")(None) == -1
    for name, _ in launches:
        assert launch(name, None) == -1, name
    h = C.c_void_p()
    assert fn("create")(C.byref(cfg), C.byref(h)) == 0
    try:
        assert h.value and fn("obs_dim")(h) == D
        assert fn("last_error")(h) == b""
        for name in ("reset", "step"):
            assert launch(name, h) == -2, name
            assert b"bind first" in fn("last_error")(h), name
            assert fn("last_error")(h).startswith(name.encode() + b": "), name
        panel = panel_cls()
        assert fn("bind")(h, C.byref(panel), None) == -1
        assert fn("bind")(None, C.byref(panel), None) == -1
        assert launch("step", h) == -2                                   # still unbound
    finally:
        fn("destroy")(h)


# one shape per step-kernel family: np32, np64, WideGeom<100>, generic np128 (> 64 KiB of LDS: the opt-in)
@pytest.mark.parametrize("n_tickers,hmax", [(30, 100), (40, 100), (100, 100), (100, 300)])
@pytest.mark.parametrize("hint_first", [True, False])
def test_stock_step_plan_is_made_off_the_step(L, n_tickers, hmax, hint_first):
    """bind, set_windows and set_desync_hint choose the step kernel and size its launch rounds.  On host
    pointers that no device owns they succeed whatever the device queries answer, before and after
    bind and in either order, and leave no error behind: the step that follows reports its own
    null arguments, not a HIP error of a query."""
    from finrl_amd import _native as nat
    cfg = nat.StockConfig(64, n_tickers, 2, 12, hmax, 1, 1, 1, 1, 0, 1e-3, 1e-3, 1e-4, 40.0)
    buf = np.zeros(4096, dtype=np.float64)                    # never read: nothing here launches
    ptr = C.c_void_p(buf.ctypes.data)
    panel, st = nat.StockPanelPtrs(ptr, ptr, ptr), nat.StockStatePtrs(ptr, ptr)

    def setters(h, hint, win):
        calls = [lambda: L.finenv_stock_set_desync_hint(h, hint),
                 lambda: L.finenv_stock_set_windows(h, win)]
        for call in (calls if hint_first else calls[::-1]):
            assert call() == 0

    h = C.c_void_p()
    assert L.finenv_stock_create(C.byref(cfg), C.byref(h)) == 0
    try:
        setters(h, 1, ptr)                                    # unbound: stored only
        assert L.finenv_stock_bind(h, C.byref(panel), C.byref(st)) == 0
        assert L.finenv_stock_last_error(h) == b""
        for hint, win in ((0, None), (1, ptr), (1, ptr), (0, ptr), (0, None)):   # every edge, and no change
            setters(h, hint, win)
            assert L.finenv_stock_last_error(h) == b""
        assert L.finenv_stock_bind(h, C.byref(panel), C.byref(st)) == 0          # a second bind plans again
        assert L.finenv_stock_step(h, None, None, None, None, None, None, 1, None) == -1
        assert L.finenv_stock_last_error(h) == b"step: null actions/obs/reward/done"
    finally:
        L.finenv_stock_destroy(h)
