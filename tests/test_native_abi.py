"""CPU-side checks of the C-ABI library: it loads (hipcc-built, no GPU needed), exports every
symbol include/finenv.h declares, the whole ctypes binding (signatures, struct layouts, constants)
agrees with that header, argument validation works, and launches fail loudly (never fall back) when no
HIP device exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import abi_header as H
from finrl_amd import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {cname: cls for cname, _, cls in nat.STRUCTS}


@pytest.fixture(scope="module")
def L():
    nat.build()
    return nat.lib()


def test_exports_every_declared_symbol(L):
    names = sorted(H.prototypes())
    assert len(names) >= 13
    for n in names:
        assert hasattr(L, n), f"libfinenv.so does not export {n}"


def test_struct_layouts_match(L):
    assert L.finenv_abi_version() == nat.ABI_VERSION == 3
    assert L.finenv_struct_size(0) == C.sizeof(nat.StockConfig)
    assert L.finenv_struct_size(1) == C.sizeof(nat.StockPanelPtrs)
    assert L.finenv_struct_size(2) == C.sizeof(nat.StockStatePtrs)
    assert H.fields("FINENV_STOCK_F64_FIELDS") == nat.STOCK_F64_FIELDS
    assert H.fields("FINENV_STOCK_I32_FIELDS") == nat.STOCK_I32_FIELDS


# ------------------------------------------------------------------ the binding against the header
def test_tables_and_header_name_the_same_functions_and_structs():
    assert set(nat.SIGNATURES) == set(H.prototypes()) and len(nat.SIGNATURES) == 116
    assert set(CLASSES) == set(H.structs()) and len(nat.STRUCTS) == len(CLASSES) == 33
    assert H.binding_errors(nat) == []


@pytest.mark.parametrize("name", sorted(H.prototypes()))
def test_signature_follows_the_prototype(L, name):
    restype, argtypes = H.expected_signature(name, CLASSES)
    fn = getattr(L, name)
    assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert nat.SIGNATURES[name] == (restype, argtypes)


@pytest.mark.parametrize("cname,which,cls", nat.STRUCTS, ids=[s[0] for s in nat.STRUCTS])
def test_struct_follows_the_header(L, cname, which, cls):
    assert cls._fields_ == H.expected_fields(cname)
    if which is not None:
        assert L.finenv_struct_size(which) == C.sizeof(cls)


def test_struct_size_gaps_stay_invalid(L):
    indexed = sorted(which for _, which, _ in nat.STRUCTS if which is not None)
    gaps = sorted(set(range(indexed[-1] + 2)) - set(indexed))
    assert gaps == [18, 22, 25, 27, 29, 32, 34]
    for which in gaps:
        assert L.finenv_struct_size(which) == -1, which


def test_field_tuples_and_constants_mirror_the_header():
    k = H.constants()
    assert len(H.FIELD_TUPLES) == 18                  # the 17 field tuples and STOPLOSS_BOOKS
    for tup in H.FIELD_TUPLES:
        assert getattr(nat, tup) == H.fields("FINENV_" + tup), tup
        assert len(getattr(nat, tup)) == k["FINENV_" + tup], tup
    for alias in ("PORTFOLIO", "CRYPTO", "STOCKNP", "TWOWAVE"):      # one enum of columns serves every env
        assert getattr(nat, alias + "_HISTORY_METRICS") is nat.STOCK_HISTORY_METRICS
    assert nat.ABI_VERSION == k["FINENV_ABI_VERSION"] and nat.FINENV_OK == k["FINENV_OK"] == 0
    # check() treats every nonzero code as an error and asks the library for its text: each has one
    errors = {n: v for n, v in k.items() if n.startswith("FINENV_ERR_")}
    assert sorted(errors.values()) == [-4, -3, -2, -1]
    for name in ("HIST_COMPLETE", "HIST_OVERFLOW", "HIST_ARMED", "AUDIT_HEAD", "AUDIT_F_LAST_DATE",
                 "AUDIT_F_CASH_SHORTAGE", "AUDIT_F_TURBULENCE", "AUDIT_F_STOP_LOSS", "AUDIT_F_LOW_PROFIT",
                 "AUDIT_F_HIGH_PROFIT", "BTC_MAX_PRICE_COLS", "VECNORM_MAX_TILES", "STOCK_MAX_TICKERS"):
        assert getattr(nat, name) == k["FINENV_" + name], name
    from finrl_amd import vec_btc, vec_stocknp
    for mod in (vec_stocknp, vec_btc):
        assert (mod.TAG_PY, mod.TAG_F32, mod.TAG_F64) == \
            (k["FINENV_NT_PY"], k["FINENV_NT_F32"], k["FINENV_NT_F64"]), mod.__name__


def test_strerror_knows_every_error_code(L):
    for name, code in H.constants().items():
        if name == "FINENV_OK" or name.startswith("FINENV_ERR_"):
            assert L.finenv_strerror(code) not in (None, b"", b"unknown error"), name


def _edited(pattern, repl):
    src = open(H.HEADER).read()
    out, n = re.subn(pattern, repl, src, count=1, flags=re.S)
    assert n == 1, pattern
    return out


# the checker can fail: each edit of the header text is reported, with the function, struct or tuple named
@pytest.mark.parametrize("pattern,repl,culprit", [
    # two same-sized fields of a struct swapped (the first such pair is finenv_stock_config's)
    (r"int32_t n_envs;(.*?)int32_t n_tickers;", r"int32_t n_tickers;\1int32_t n_envs;", "finenv_stock_config"),
    # one argument dropped from a prototype
    (r"(finenv_stock_step\([^)]*?), int32_t auto_reset", r"\1", "finenv_stock_step"),
    # an int32_t argument changed to double
    (r"(finenv_stock_init\(finenv_stock \*h, )int32_t", r"\1double", "finenv_stock_init"),
    # an enumerator inserted in the middle of a field enum
    (r"(FINENV_SF_COST,)", r"\1 FINENV_SF_EXTRA,", "STOCK_F64_FIELDS"),
    # a prototype added with no table entry
    (r"(int\s+finenv_struct_size\(int which\);)", r"\1\nint finenv_stock_new_call(finenv_stock *h);",
     "finenv_stock_new_call"),
], ids=["fields-swapped", "argument-dropped", "int32-to-double", "enumerator-inserted", "prototype-added"])
def test_checker_reports_an_edited_header(pattern, repl, culprit):
    errs = H.binding_errors(nat, _edited(pattern, repl))
    assert len(errs) == 1 and errs[0].startswith(culprit + ": "), errs


class _EarlierBuild:
    """The real library as a build from before `hidden` existed: those symbols are missing, and
    finenv_struct_size answers -1 past the v3 baseline (and `sizes` where a test says otherwise)."""

    def __init__(self, L, hidden, sizes=()):
        self._L, self._hidden, sizes = L, hidden, dict(sizes)
        # (a plain function: declare() sets restype / argtypes on it like on any other entry point)
        self.finenv_struct_size = lambda which: sizes.get(
            which, -1 if which > 17 else L.finenv_struct_size(which))

    def __getattr__(self, name):
        if name.startswith(self._hidden):
            raise AttributeError(name)
        return getattr(self._L, name)


@pytest.mark.parametrize("hidden", [("finenv_btc_",), ("finenv_replay_", "finenv_rollout_", "finenv_vecnorm_"),
                                    ("finenv_vecnorm_",)])
def test_an_earlier_build_still_declares_and_checks(L, hidden):
    old = _EarlierBuild(L, hidden)
    assert not hasattr(old, hidden[0] + "step") and hasattr(old, "finenv_stock_step")
    assert nat.declare(old) is old
    with pytest.raises(nat.NativeLibraryError, match="StockNpConfig"):      # the baseline must match
        nat.declare(_EarlierBuild(L, hidden, {9: C.sizeof(nat.StockNpConfig) + 8}))
    with pytest.raises(nat.NativeLibraryError, match="StockPanelPtrs"):     # ... and -1 is no answer there
        nat.declare(_EarlierBuild(L, hidden, {1: -1}))
    with pytest.raises(nat.NativeLibraryError, match="BtcConfig"):          # past it, only -1 or sizeof
        nat.declare(_EarlierBuild(L, hidden, {19: C.sizeof(nat.BtcConfig) + 8}))


def test_create_validates_arguments(L):
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


# One valid config per handle kind, the obs_dim it gives, and the entry points that launch work (their
# argument counts come from the header).  The host contract below holds for every kind alike.
def _kind_cases():
    cash = (64, 4, 3, 50, 0, 1, 0, 0, 10.0, 3e-3, 3e-3, 1e6, 0.1, 0.0)
    return {
        "stock": (nat.StockConfig(64, 30, 8, 100, 100, 0, 1, 1, 1, 0, 1e-3, 1e-3, 1e-4, 0.0),
                  nat.StockPanelPtrs, 301,
                  ("init", "reset", "observe", "refresh", "step", "episode_stats", "last_episode_stats")),
        "portfolio": (nat.PortfolioConfig(64, 5, 4, 50, 1e6), nat.PortfolioPanelPtrs, 45,
                      ("reset", "step", "last_episode_stats")),
        "crypto": (nat.CryptoConfig(64, 3, 4, 50, 2, 0, 1e6, 1e-3, 1e-3, 0.99),
                   nat.CryptoPanelPtrs, 12, ("reset", "step", "step_record")),
        "stocknp": (nat.StockNpConfig(64, 5, 7, 50, 10, 0, 100.0, 1e-3, 1e-3, 2 ** -11, 0.99, 0.0),
                    nat.StockNpPanelPtrs, 25, ("reset", "step")),
        "cashpenalty": (nat.CashPenaltyConfig(*cash), nat.CashPenaltyPanelPtrs, 17, ("reset", "step")),
        "stoploss": (nat.StopLossConfig(*cash, 0.9, 1.2), nat.StopLossPanelPtrs, 17, ("reset", "step")),
    }


@pytest.mark.parametrize("kind", ["stock", "portfolio", "crypto", "stocknp", "cashpenalty", "stoploss"])
def test_host_contract_every_kind(L, kind):
    """Null handles, create / obs_dim, launches before bind and bind with a null state pointer give
    the same codes and messages in every env's C ABI (no GPU needed: nothing here launches)."""
    cfg, panel_cls, D, launches = _kind_cases()[kind]
    fn = lambda name: getattr(L, f"finenv_{kind}_{name}")          # noqa: E731

    def launch(name, h):        # a private function object: the library's own argtypes stay as declared
        f = L[f"finenv_{kind}_{name}"]
        nargs = len(H.prototypes()[f"finenv_{kind}_{name}"][1]) - 1          # the arguments after the handle
        f.argtypes = [C.c_void_p] * (1 + nargs)
        return f(h, *([None] * nargs))

    assert fn("last_error")(None) == b"null handle"
    assert fn("obs_dim")(None) == -1
    for name in launches:
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
