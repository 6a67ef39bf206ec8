"""The finenv_btc_* family of the C ABI and the host side of VecBitcoinEnv, without a GPU: nothing
here launches."""
import ctypes as C
import os

import numpy as np
import pytest

import abi_header as H
import btc_model as bm


@pytest.fixture(scope="module")
def L():
    from finrl_amd import _native
    _native.build()
    return _native.lib()


def _cfg(nat, E=64, P=2, W=8, T=50):
    return nat.BtcConfig(E, P, W, T, 0, 0, 1e6, 1e-3, 0.99)


def test_every_declared_symbol_is_exported(L):
    names = {n for n in H.prototypes() if n.startswith("finenv_btc_")}
    assert names == {"finenv_btc_" + n for n in ("create", "destroy", "last_error", "obs_dim", "bind",
                                                  "reset", "step", "set_windows")}
    for n in names:
        assert hasattr(L, n), n
    assert H.constants()["FINENV_ABI_VERSION"] == 3 and L.finenv_abi_version() == 3


def test_struct_sizes_and_field_order(L):
    from finrl_amd import _native as nat
    for which, cls in ((19, nat.BtcConfig), (20, nat.BtcPanelPtrs), (21, nat.BtcStatePtrs)):
        assert L.finenv_struct_size(which) == C.sizeof(cls), cls.__name__
    assert L.finenv_struct_size(18) == -1 and L.finenv_struct_size(22) == -1
    assert all(n.startswith("FINENV_BF_") for n in H.enum("FINENV_BTC_F64_FIELDS")[:-1])
    assert H.fields("FINENV_BTC_F64_FIELDS") == nat.BTC_F64_FIELDS
    assert all(n.startswith("FINENV_BI_") for n in H.enum("FINENV_BTC_I32_FIELDS")[:-1])
    assert H.fields("FINENV_BTC_I32_FIELDS") == nat.BTC_I32_FIELDS
    cfg = H.structs()["finenv_btc_config"]
    assert all(t in ("int32_t", "double") for t, _ in cfg)
    assert [f for _, f in cfg] == [f[0] for f in nat.BtcConfig._fields_]
    assert H.constants()["FINENV_BTC_MAX_PRICE_COLS"] == nat.BTC_MAX_PRICE_COLS


def test_host_contract(L):
    """The codes and messages of test_native_abi.test_host_contract_every_kind, for kind btc."""
    from finrl_amd import _native as nat
    launches = ("reset", "step")

    def launch(name, h):        # a private function object: the library's own argtypes stay as declared
        f = L[f"finenv_btc_{name}"]
        nargs = len(H.prototypes()[f"finenv_btc_{name}"][1]) - 1             # the arguments after the handle
        f.argtypes = [C.c_void_p] * (1 + nargs)
        return f(h, *([None] * nargs))

    assert L.finenv_btc_last_error(None) == b"null handle"
    assert L.finenv_btc_obs_dim(None) == -1
    for name in launches:
        assert launch(name, None) == -1, name
    assert L.finenv_btc_set_windows(None, None) == -1
    h = C.c_void_p()
    cfg = _cfg(nat)
    assert L.finenv_btc_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert h.value and L.finenv_btc_obs_dim(h) == 2 + 9
        assert L.finenv_btc_last_error(h) == b""
        for name in ("reset", "step"):
            assert launch(name, h) == -2, name
            assert L.finenv_btc_last_error(h) == name.encode() + b": bind first"
        # windows: attach before bind, NULL detaches
        win = np.zeros((2, 64), np.int32)
        assert L.finenv_btc_set_windows(h, win.ctypes.data_as(C.c_void_p)) == 0
        assert L.finenv_btc_set_windows(h, None) == 0
        assert launch("step", h) == -2
        panel = nat.BtcPanelPtrs()
        assert L.finenv_btc_bind(h, C.byref(panel), None) == -1
        assert L.finenv_btc_bind(None, C.byref(panel), None) == -1
        state = nat.BtcStatePtrs()
        assert L.finenv_btc_bind(h, C.byref(panel), C.byref(state)) == -1
        assert L.finenv_btc_last_error(h) == b"bind: null pointer"
        assert launch("step", h) == -2                                   # still unbound
    finally:
        L.finenv_btc_destroy(h)
    L.finenv_btc_destroy(None)


@pytest.mark.parametrize("bad", [dict(E=0), dict(E=-3), dict(P=0), dict(P=246), dict(W=6), dict(T=1)])
def test_create_rejects(L, bad):
    from finrl_amd import _native as nat
    h = C.c_void_p(1)
    cfg = _cfg(nat, **bad)
    assert L.finenv_btc_create(C.byref(cfg), C.byref(h)) == -1
    assert not h.value
    ok = _cfg(nat, P=245, W=7, T=2, E=1)
    assert L.finenv_btc_create(C.byref(ok), C.byref(h)) == 0 and L.finenv_btc_obs_dim(h) == 254
    L.finenv_btc_destroy(h)
    assert L.finenv_btc_create(None, C.byref(h)) == -1 and L.finenv_btc_create(C.byref(ok), None) == -1


def test_no_cpu_path_and_input_contract():
    from finrl_amd import _native as nat
    from finrl_amd.vec_btc import VecBitcoinEnv
    price, tech = np.full((6, 1), 300.0), np.zeros((6, 7))
    with pytest.raises(nat.FinenvError, match="no CPU path"):
        VecBitcoinEnv(price, tech, 4, device="cpu")
    for p, t, exc in ((price.astype(np.float32), tech, TypeError), (price, tech.astype(np.float32), TypeError),
                      (price.tolist(), tech, TypeError), (price, tech[:, :6], ValueError),
                      (price[:1], tech[:1], ValueError), (price, tech[:5], ValueError),
                      (price[:, 0], tech, ValueError)):
        with pytest.raises(exc):
            VecBitcoinEnv(p, t, 4, device="cuda")


def test_facade_modes_and_registration():
    from finrl_amd.distributed import env_class
    from finrl_amd.meta.env_cryptocurrency_trading.env_btc_ccxt import BitcoinEnv
    from finrl_amd.vec_btc import VecBitcoinEnv
    import finrl_amd
    assert env_class("btc") is VecBitcoinEnv is finrl_amd.VecBitcoinEnv
    price, tech = np.full((30, 1), 300.0), np.zeros((30, 7))
    with pytest.raises(ValueError, match="^Invalid Mode!$"):
        BitcoinEnv(price_ary=price, tech_ary=tech, mode="live")
    with pytest.raises(ValueError, match="^Data files not found!$"):
        BitcoinEnv(data_cwd=os.path.join(H.ROOT, "no_such_directory"))


def test_mode_panel_equals_load_data():
    """The three windows of mode_panel's panel hold the arrays the reference's load_data gave the
    three reference envs of btc_modes."""
    from finrl_amd.vec_btc import VecBitcoinEnv, mode_arrays, mode_panel
    modes = bm.load_fixture("btc_modes")
    kw = modes["train"]["kwargs"]
    split = [kw[k] for k in ("time_frequency", "start", "mid1", "mid2", "end")]
    raw_p, raw_t = modes["train"]["raw_price"], modes["train"]["raw_tech"]
    price, tech, win = mode_panel(raw_p, raw_t, *split)
    assert VecBitcoinEnv.mode_panel is mode_panel
    assert price.dtype == tech.dtype == np.float64 and price.shape[0] == tech.shape[0]
    at = 0
    for mode in ("train", "test", "trade"):
        s, t = win[mode]
        assert s == at and t - s == modes[mode]["price_ary"].shape[0] >= 2
        assert np.array_equal(price[s:t], modes[mode]["price_ary"])
        assert np.array_equal(tech[s:t], modes[mode]["tech_ary"])
        p, q = mode_arrays(raw_p, raw_t, *split)[mode]
        assert np.array_equal(p, price[s:t]) and np.array_equal(q, tech[s:t])
        at = t
    assert at == price.shape[0]


def test_obs_template_is_the_reference_observation():
    """Columns 1 .. D-2 of every recorded observation are the host-evaluated template row."""
    from finrl_amd.vec_btc import obs_template
    for name in ("btc_basic", "btc_wide", "btc_modes"):
        for case, c in bm.load_fixture(name).items():
            tmpl = obs_template(c["price_ary"], c["tech_ary"])
            assert tmpl.dtype == np.float32 and tmpl.shape[1] == c["obs"].shape[1] - 2
            day = 0
            for i, op in enumerate(c["ops"]):
                day = 0 if op == bm.OP_RESET else day + 1
                assert np.array_equal(tmpl[day].view(np.uint32), c["obs"][i, 1:-1].view(np.uint32)), (case, i)
