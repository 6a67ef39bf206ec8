"""Device-resident episode history of the HIP cash-penalty and stop-loss envs
(finenv_{cashpenalty,stoploss}_set_history, VecCashPenaltyEnv.enable_history):

  * exact against the recording rule of include/finenv.h applied on the host to the audit row read back
    after every step -- the row the single-env facades already pin to the reference;
  * exact against one CPU oracle per env on its slice of the panel, without the audit row;
  * the reference's save_asset_memory() / save_action_memory() frames (tests/golden/harness_sb3_*.npz)
    for envs that run the fixture as a window of a NaN-padded panel among other envs, at the facades'
    tolerances, and exactly against the facade's own frames;
  * arming, resets, auto-reset, overflow, detaching, the optional tensors, graph capture;
  * metrics() against pandas; a transactions slab past 4 GiB.

E = 300: two blocks of the record kernel (the second partial) and a partial 64-env step block."""
import contextlib
import io
import os

import numpy as np
import pytest

import harness_loops as hl
from twowave_windows_cases import COMMON, KINDS, classes, make_panel, nan_padded

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_ENVS, T_ROWS = 300, 24
ARMED, COMPLETE, OVERFLOW = 4, 1, 2
F_LAST, F_SHORT, F_STOP = 1, 2, 8
# every step-kernel form (rows of 61, 181 and 331 columns at N = 30), both action forms, patient and
# not, with and without windows, turbulence on and off
CASES = [
    dict(N=1, C=2, disc=False, patient=False, win=True, thr=None),
    dict(N=5, C=2, disc=True, patient=True, win=False, thr=40.0),
    dict(N=30, C=1, disc=False, patient=True, win=True, thr=None),
    dict(N=30, C=5, disc=True, patient=False, win=True, thr=40.0),
    dict(N=30, C=5, disc=False, patient=False, win=False, thr=None),
    dict(N=30, C=10, disc=True, patient=False, win=False, thr=None),
    dict(N=30, C=10, disc=False, patient=True, win=True, thr=40.0),
    dict(N=32, C=1, disc=True, patient=False, win=True, thr=None),
]
CASE_IDS = [f"n{c['N']}c{c['C']}-{'disc' if c['disc'] else 'cont'}-{'patient' if c['patient'] else 'plain'}"
            f"-{'win' if c['win'] else 'panel'}" for c in CASES]
SERIES = ("cash", "asset_value", "reward", "reason")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _kwargs(case):
    # dollars per trade so that a full-size action stream spends the cash within a few steps
    return dict(hmax=2.5e6 / case["N"], turbulence_threshold=case["thr"], patient=case["patient"],
                discrete_actions=case["disc"], **COMMON)


def _windows(rng, case, E=E_ENVS, T=T_ROWS):
    """Per-env windows of 2 .. T rows (two of one row), or None for the whole panel."""
    if not case["win"]:
        return None
    length = rng.integers(2, T + 1, E)
    length[[1, E - 1]] = 1
    s = rng.integers(0, T - length + 1)
    return s.astype(np.int64), (s + length).astype(np.int64)


def _actions(rng, E, N):
    """A different stream per env: full-size actions run out of cash within a few steps, the small ones
    of every fourth env reach the last date."""
    a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
    scale = np.array([0.004, 0.05, 0.3, 1.0], np.float32)[np.arange(E) % 4]
    return a * scale[:, None]


def _make(kind, case, auto, windows, E=E_ENVS, T=T_ROWS, **kw):
    Panel, Env, _ = classes(kind)
    close, info, turb = make_panel(case["N"], case["C"], T)
    env = Env(Panel(close, info, turb), E, random_start=False, auto_reset=auto, windows=windows,
              **_kwargs(case), **kw)
    return env, (close, info, turb)


class HostRecord:
    """The recording rule of include/finenv.h on host arrays laid out as the device holds them."""

    def __init__(self, E, N, cap):
        self.E, self.cap = E, cap
        self.cash, self.asset_value, self.reward = (np.zeros((cap, E)) for _ in range(3))
        self.reason = np.zeros((cap, E), np.int32)
        self.tx, self.actions = np.zeros((cap, E, N)), np.zeros((cap, E, N), np.float32)
        self.start, self.end, self.ntx, self.length, self.flags = (np.zeros(E, np.int32) for _ in range(5))
        self.n_last = self.n_short_end = self.n_patient_short = self.n_stop = 0

    def arm(self, mask, date_index, end):
        m = np.ones(self.E, bool) if mask is None else np.asarray(mask, bool)
        self.length[m], self.ntx[m], self.flags[m] = 0, 0, ARMED
        self.start[m], self.end[m] = np.asarray(date_index)[m], np.asarray(end)[m]

    def record(self, audit, actions, done):
        for e in range(self.E):
            fl = self.flags[e]
            if not fl & ARMED or fl & COMPLETE:
                continue
            reason = int(audit[e, 3])
            if reason & F_LAST:
                self.flags[e] |= COMPLETE
                self.n_last += 1
                continue
            k = self.length[e]
            if k == self.cap:
                self.flags[e] |= OVERFLOW | (COMPLETE if done[e] else 0)
                continue
            self.cash[k, e], self.asset_value[k, e], self.reward[k, e] = audit[e, :3]
            self.reason[k, e] = reason
            self.actions[k, e] = actions[e]
            if not (reason & F_SHORT and done[e]):
                self.tx[k, e] = audit[e, 4:]
                self.ntx[e] += 1
            self.length[e] = k + 1
            self.n_short_end += bool(reason & F_SHORT and done[e])
            self.n_patient_short += bool(reason & F_SHORT and not done[e])
            self.n_stop += bool(reason & F_STOP)
            if done[e]:
                self.flags[e] |= COMPLETE

    def assert_equal(self, hist, tag, tx=True, actions=True):
        """Every per-env word and every entry below ``len`` (transactions: below ``ntx``), exactly."""
        for k in ("start", "end", "ntx", "length", "flags"):
            np.testing.assert_array_equal(getattr(hist, k).cpu().numpy(), getattr(self, k), err_msg=f"{k} {tag}")
        live = np.arange(self.cap)[:, None] < self.length[None, :]
        for k in SERIES:
            np.testing.assert_array_equal(getattr(hist, k).cpu().numpy()[live], getattr(self, k)[live],
                                          err_msg=f"{k} {tag}")
        if actions:
            np.testing.assert_array_equal(hist.actions.cpu().numpy()[live], self.actions[live],
                                          err_msg=f"actions {tag}")
        if tx:
            live = np.arange(self.cap)[:, None] < self.ntx[None, :]
            np.testing.assert_array_equal(hist.tx.cpu().numpy()[live], self.tx[live], err_msg=f"tx {tag}")


def _arm_host(rec, env, mask=None):
    end = env.active_windows[1].cpu().numpy() if env.active_windows is not None else \
        np.full(env.num_envs, env.panel.T)
    rec.arm(mask, env.state["date_index"].cpu().numpy(), end)


def _step_both(env, rec, a):
    _, _, done, _ = env.step(_dev(a))
    rec.record(env.audit.cpu().numpy(), a, done.cpu().numpy().astype(bool))
    return done.cpu().numpy().astype(bool)


def _poison(hist):
    """Junk in every tensor of the record that holds entries: an entry the kernel should have written
    and did not, or wrote into the wrong place, then shows."""
    for k in SERIES + ("tx", "actions"):
        t = getattr(hist, k)
        if t is not None:
            t.fill_(-7)


# ------------------------------------------------------------------------------------------
# 1. exact against the audit row
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_record_equals_the_rule_applied_to_the_audit_row(kind, case):
    _need_gpu()
    E, N = E_ENVS, case["N"]
    for auto in (True, False):
        rng = np.random.default_rng(17 + N + case["C"])
        env, _ = _make(kind, case, auto, _windows(rng, case))
        env.set_next_start(rng.integers(0, 4, E).astype(np.int32))
        env.reset()
        hist = env.enable_history()
        assert hist is env.history and env.enable_history(capacity=3) is hist and env.audit is not None
        assert hist.capacity == env.max_step + 1 and (case["win"] or hist.capacity == T_ROWS)
        _poison(hist)
        rec = HostRecord(E, N, hist.capacity)
        _arm_host(rec, env)                                  # the constructor armed every env
        rec.assert_equal(hist, "armed")
        assert bool(hist.armed.all()) and not bool(hist.complete.any())
        for s in range(T_ROWS + 4):                          # past every episode's end
            done = _step_both(env, rec, _actions(rng, E, N))
            if s in (2, 11):
                rec.assert_equal(hist, f"auto={auto} step {s}")
            if not auto and s == 13 and done.any():          # a host reset arms exactly its envs
                env.reset(_dev(done.astype(np.uint8)))
                _arm_host(rec, env, done)
        rec.assert_equal(hist, f"auto={auto} end")
        np.testing.assert_array_equal(hist.complete.cpu().numpy(), (rec.flags & COMPLETE) != 0)
        assert not bool(hist.overflow.any())
        # the inputs reach both endings (patient: the shortage that does not end the episode)
        assert rec.n_last > 0
        if case["patient"]:
            assert rec.n_patient_short > 0 and rec.n_short_end == 0
        else:
            assert rec.n_short_end > 0
            assert ((rec.ntx == rec.length - 1) & (rec.length > 0)).any()
        if kind == "stoploss":
            assert rec.n_stop > 0                            # forced sales on the volatile panel
        if auto:
            assert (rec.flags & COMPLETE).all()              # every record is final, and was kept


# ------------------------------------------------------------------------------------------
# 2. exact against one oracle per env, without the audit row
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_record_equals_one_oracle_per_env(kind, case):
    _need_gpu()
    E, N, T = E_ENVS, case["N"], T_ROWS
    Oracle = classes(kind)[2]
    for auto in (True, False):
        rng = np.random.default_rng(29 + N + case["C"])
        win = _windows(rng, case)
        env, (close, info, turb) = _make(kind, case, auto, win)
        ws, wt = win if win is not None else (np.zeros(E, np.int64), np.full(E, T, np.int64))
        off = rng.integers(0, 4, E).astype(np.int32)
        env.set_next_start(off)
        env.reset()
        hist = env.enable_history()
        _poison(hist)
        orc = [Oracle(close[s:t], info[s:t], turb[s:t], n_envs=1, **_kwargs(case)) for s, t in zip(ws, wt)]
        for e, o in enumerate(orc):
            o.reset(int(min(off[e], wt[e] - ws[e] - 1)))
        cash, total, reward, rows = ([[] for _ in range(E)] for _ in range(4))
        live = np.ones(E, bool)
        ended_short = np.zeros(E, bool)
        for s in range(T + 2):
            a = _actions(rng, E, N)
            env.step(_dev(a))
            for e in np.flatnonzero(live):
                o = orc[e]
                before = o.state()
                di = int(before["date_index"][0])
                _, r, d = o.step(a[e:e + 1])
                if di == wt[e] - ws[e] - 1:                  # the last date appends nothing
                    assert d[0]
                    live[e] = False
                    continue
                cash[e].append(before["coh"][0])
                total[e].append(o.state()["logged_total"][0])
                reward[e].append(r[0])
                rows[e].append(ws[e] + di)
                if d[0]:
                    live[e], ended_short[e] = False, True
        assert not live.any()
        length = hist.length.cpu().numpy()
        np.testing.assert_array_equal(length, [len(c) for c in cash])
        np.testing.assert_array_equal(hist.ntx.cpu().numpy(), length - ended_short)
        h_cash, h_av, h_rew = (getattr(hist, k).cpu().numpy() for k in ("cash", "asset_value", "reward"))
        got_rows = hist.rows(list(range(E)))
        for e in range(E):
            n = length[e]
            np.testing.assert_array_equal(h_cash[:n, e], cash[e], err_msg=f"cash env {e}")
            np.testing.assert_array_equal(h_cash[:n, e] + h_av[:n, e], total[e], err_msg=f"total env {e}")
            np.testing.assert_array_equal(h_rew[:n, e], reward[e], err_msg=f"reward env {e}")
            np.testing.assert_array_equal(got_rows[e], rows[e], err_msg=f"rows env {e}")
        np.testing.assert_array_equal(hist.end.cpu().numpy(), wt)
        assert bool(hist.complete.all())
        assert ended_short.any() != case["patient"] and not ended_short.all()


# ------------------------------------------------------------------------------------------
# 3. the reference's frames, for envs among others of one batch
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sb3_cashpenalty", "sb3_cashpenalty_patient", "sb3_stoploss",
                                  "sb3_stoploss_patient"])
def test_reference_frames_from_a_window_of_a_nan_padded_panel(name):
    _need_gpu()
    import test_gpu_harness as th
    kind = "stoploss" if "stoploss" in name else "cashpenalty"
    Panel, Env, _ = classes(kind)
    z = np.load(os.path.join(GOLDEN, f"harness_{name}.npz"), allow_pickle=False)
    T, N, Cc, disc, inc, use_t, patient, _ = z["cfg_int"].tolist()
    cf = z["cfg_float"].tolist()
    kw = dict(buy_cost_pct=cf[1], sell_cost_pct=cf[2], hmax=cf[0], discrete_actions=bool(disc),
              shares_increment=inc, turbulence_threshold=cf[5] if use_t else None, initial_amount=cf[3],
              cash_penalty_proportion=cf[4], patient=bool(patient))
    if kind == "stoploss":
        kw.update(stoploss_penalty=cf[6], profit_loss_ratio=cf[7])
    block = (z["close"], z["info"], z["turb"])
    close, info, turb, offs = nan_padded([block, block], 3, N, Cc)
    fixture_dates = [f"2020-{1 + t // 28:02d}-{1 + t % 28:02d}" for t in range(T)]
    dates = [f"pad{r}" for r in range(len(close))]
    dates[offs[0]:offs[0] + T] = fixture_dates
    E, mine = E_ENVS, (3, 280)                               # one env in each block of the record kernel
    w0 = np.full(E, offs[1])
    w0[list(mine)] = offs[0]
    env = Env(Panel(close, info, turb, dates=dates), E, random_start=False, auto_reset=False,
              windows=(w0, w0 + T), **kw)
    env.set_next_start(0)
    obs = env.reset().cpu().numpy()
    hist = env.enable_history()
    cols = 1 + N + Cc * np.arange(N)
    models = [hl.ScriptedModel(z["base"], cols) for _ in mine]
    rng = np.random.default_rng(5)
    acct = acts = None
    for i in range(T):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32) * np.float32(0.01)
        for m, e in zip(models, mine):
            a[e] = m.predict(obs[e:e + 1])[0][0]
        obs, _, done, _ = env.step(_dev(a))
        obs, done = obs.cpu().numpy(), done.cpu().numpy()
        if i == T - 2:
            acct, acts = hist.save_asset_memory(list(mine)), hist.save_action_memory(list(mine))
        if done[mine[0]]:
            break
    assert i == T - 1 and models[0].step == int(z["model_steps"])
    with contextlib.redirect_stdout(io.StringIO()):
        facade, _, _ = th._dollar_env(z, "sb3_" + kind)
        f_acct, f_acts = hl.drl_prediction(hl.ScriptedModel(z["base"], cols), facade)
    for am, ac in zip(acct, acts):
        assert am["date"].tolist() == z["account_date"].tolist()
        assert ac["date"].tolist() == z["action_date"].tolist()
        for k in ("cash", "asset_value", "total_assets", "reward"):
            np.testing.assert_allclose(am[k].to_numpy(np.float64), z[f"account_{k}"], rtol=1e-12,
                                       atol=1e-15, err_msg=k)
        np.testing.assert_allclose(np.stack(ac["actions"].tolist()), z["action_actions"], rtol=1e-15, atol=0)
        np.testing.assert_allclose(np.stack(ac["transactions"].tolist()), z["action_transactions"],
                                   rtol=1e-12, atol=1e-12)
        # the facade on the same frame: exactly
        assert am.columns.tolist() == f_acct.columns.tolist() and ac.columns.tolist() == f_acts.columns.tolist()
        assert am.equals(f_acct)
        assert ac["date"].tolist() == f_acts["date"].tolist()
        for k in ("actions", "transactions"):
            got, want = np.stack(ac[k].tolist()), np.stack(f_acts[k].tolist())
            assert got.dtype == want.dtype, k
            np.testing.assert_array_equal(got, want, err_msg=k)
    np.testing.assert_array_equal(hist.rows(mine[1]), offs[0] + np.arange(T - 1))


# ------------------------------------------------------------------------------------------
# 4. lifecycle
# ------------------------------------------------------------------------------------------
LIFE = dict(N=5, C=2, disc=False, patient=False, win=True, thr=None)


@pytest.mark.parametrize("kind", KINDS)
def test_arm_and_reset_by_mask(kind):
    _need_gpu()
    E, N = E_ENVS, LIFE["N"]
    rng = np.random.default_rng(41)
    env, _ = _make(kind, LIFE, False, _windows(rng, LIFE))
    env.reset()
    hist = env.enable_history()
    rec = HostRecord(E, N, hist.capacity)
    _arm_host(rec, env)
    for s in range(14):
        _step_both(env, rec, _actions(rng, E, N) * np.float32(0.02))
        if s == 3:                                           # mid-episode: an empty record from here on
            m = rng.random(E) < 0.4
            hist.arm(m)
            _arm_host(rec, env, m)
            rec.assert_equal(hist, "arm(mask)")
            assert (rec.start[m] > env.state["start"].cpu().numpy()[m]).any()
        if s == 8:                                           # reset(mask) arms only the envs of the mask
            m = rng.random(E) < 0.5
            before = hist.length.clone()
            env.reset(_dev(m.astype(np.uint8)))
            _arm_host(rec, env, m)
            rec.assert_equal(hist, "reset(mask)")
            assert bool((hist.length[_dev(~m)] == before[_dev(~m)]).all()) and int(hist.length[_dev(m)].max()) == 0
    rec.assert_equal(hist, "end")
    assert rec.length.max() > 5


@pytest.mark.parametrize("kind", KINDS)
def test_overflow_keeps_the_entries_below_the_capacity(kind):
    _need_gpu()
    E, N, cap = E_ENVS, LIFE["N"], 4
    rng = np.random.default_rng(43)
    env, _ = _make(kind, LIFE, True, None)
    env.reset()
    hist = env.enable_history(capacity=cap)
    _poison(hist)
    rec = HostRecord(E, N, cap)
    _arm_host(rec, env)
    guard = {k: getattr(hist, k).clone() for k in ("tx", "actions")}
    for s in range(T_ROWS + 2):
        _step_both(env, rec, _actions(rng, E, N))
    rec.assert_equal(hist, "overflow")
    over = hist.overflow.cpu().numpy()
    assert over.any() and not over.all() and (rec.length[over] == cap).all()
    assert bool(hist.complete.all())
    # an env that ran out of cash on its first step holds one entry: rows 1 .. of its columns are untouched
    short = np.flatnonzero(rec.length == 1)
    assert len(short)
    for k, t in guard.items():
        assert torch.equal(getattr(hist, k)[1:, _dev(short)], t[1:, _dev(short)]), k


@pytest.mark.parametrize("kind", KINDS)
def test_detach_optional_tensors_and_missing_audit(kind):
    _need_gpu()
    from finrl_amd import _native as nat
    E, N = E_ENVS, LIFE["N"]
    rng = np.random.default_rng(47)
    # transactions=False / actions=False: the scalars and the counters are recorded all the same
    for tx, act in ((False, True), (True, False), (False, False)):
        env, _ = _make(kind, LIFE, True, None)
        env.reset()
        hist = env.enable_history(transactions=tx, actions=act)
        assert (hist.tx is None) == (not tx) and (hist.actions is None) == (not act)
        rec = HostRecord(E, N, hist.capacity)
        _arm_host(rec, env)
        for s in range(6):
            _step_both(env, rec, _actions(rng, E, N))
        rec.assert_equal(hist, f"tx={tx} actions={act}", tx=tx, actions=act)
        assert hist.save_asset_memory(0) is not None
        with pytest.raises(nat.FinenvError, match="=False"):
            hist.save_action_memory(0)
    # set_history(None) stops recording; the attached tensors keep what they hold
    env._call("set_history", None)
    keep = {k: getattr(hist, k).clone() for k in SERIES + ("length", "ntx", "flags")}
    env.step(_dev(_actions(rng, E, N) * np.float32(0.01)))
    for k, t in keep.items():
        assert torch.equal(getattr(hist, k), t), k
    with pytest.raises(nat.FinenvError, match="no history attached"):
        hist.arm()
    # a history without the audit block it copies from: the step refuses
    env2, _ = _make(kind, LIFE, True, None)
    env2.reset()
    env2.enable_history()
    env2._call("set_audit", None)
    with pytest.raises(nat.FinenvError, match="history needs an audit block"):
        env2.step(_dev(_actions(rng, E, N)))
    env2._call("set_audit", env2.audit.data_ptr())
    env2.step(_dev(_actions(rng, E, N)))
    assert int(env2.history.length.max()) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_with_windows_redrawn_on_done_equals_eager(kind):
    """step + a redraw of the pending windows of the envs that reported done, captured as one graph and
    replayed, against the same sequence launched eagerly on a second env."""
    _need_gpu()
    E, N, T = E_ENVS, LIFE["N"], T_ROWS
    rng = np.random.default_rng(53)
    win = _windows(rng, LIFE)
    envs = []
    for _ in range(2):
        env, _ = _make(kind, LIFE, True, win)
        env.reset()
        env.enable_history(capacity=T)                       # before the capture: launch arguments
        envs.append(env)
    graph_env, eager_env = envs
    act = torch.zeros(E, N, device="cuda")
    new_s = torch.zeros(E, dtype=torch.int32, device="cuda")
    new_t = torch.ones(E, dtype=torch.int32, device="cuda")

    def body(env):
        env.step(act)
        env.set_windows(new_s, new_t, mask=env.done)

    def feed():
        length = rng.integers(2, T + 1, E)
        s = rng.integers(0, T - length + 1)
        act.copy_(torch.from_numpy(_actions(rng, E, N)))
        new_s.copy_(torch.from_numpy(s.astype(np.int32)))
        new_t.copy_(torch.from_numpy((s + length).astype(np.int32)))

    feed()
    side = torch.cuda.Stream()                               # one eager run first (caches, allocations)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body(graph_env)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    body(eager_env)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(graph_env)
    body(eager_env)                                          # (the capture launched nothing)
    g.replay()
    for rep in range(2 * T):
        if rep == T:                                         # every env onto its redrawn window, armed again
            first = graph_env.history.length.clone()
            for env in envs:
                env.reset()
        feed()
        g.replay()
        body(eager_env)
    torch.cuda.synchronize()
    hg, he = graph_env.history, eager_env.history
    assert bool(hg.complete.all()) and int(first.max()) > 3 and int(hg.length.max()) > 3
    assert torch.equal(graph_env.active_windows, eager_env.active_windows)
    assert not torch.equal(hg.end, _dev(win[1].astype(np.int32)))            # recorded on redrawn windows
    for k in ("start", "end", "ntx", "length", "flags"):
        assert torch.equal(getattr(hg, k), getattr(he, k)), k
    live = torch.arange(hg.capacity, device="cuda")[:, None] < hg.length[None, :]
    for k in SERIES + ("actions",):
        assert torch.equal(getattr(hg, k)[live], getattr(he, k)[live]), k
    live = torch.arange(hg.capacity, device="cuda")[:, None] < hg.ntx[None, :]
    assert torch.equal(hg.tx[live], he.tx[live])


# ------------------------------------------------------------------------------------------
# 5. metrics
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_metrics_against_pandas(kind):
    _need_gpu()
    import pandas as pd
    E, N = E_ENVS, LIFE["N"]
    rng = np.random.default_rng(59)
    env, _ = _make(kind, LIFE, True, None)
    env.reset()
    hist = env.enable_history()
    flat = np.arange(E) % 5 == 2                             # no trades: a constant account value
    for s in range(T_ROWS):
        a = _actions(rng, E, N)
        a[flat] = 0
        env.step(_dev(a))
    hist.flags[7] = 0                                        # an env that was never armed
    m = hist.metrics().cpu().numpy()
    d = {k: v.cpu().numpy() for k, v in hist.metrics_dict(4 ** 0.5).items()}
    assert list(d) == list(hist.metric_keys) == ["n_returns", "cumulative_return", "mean", "std", "sharpe",
                                                 "max_drawdown"]
    length = hist.length.cpu().numpy()
    total = (hist.cash + hist.asset_value).cpu().numpy()
    assert (length == 1).any() and (length > 5).any()
    for e in range(E):
        if e == 7 or length[e] == 0:                         # unarmed, or armed and empty
            assert np.isnan(m[e]).all() and np.isnan(d["mean"][e])
            continue
        v = pd.Series(total[:length[e], e])
        r = v.pct_change().dropna()
        assert m[e, 0] == len(r) == length[e] - 1
        np.testing.assert_allclose(m[e, 1], v.iloc[-1] / v.iloc[0] - 1, rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(m[e, 5], (v / v.cummax() - 1).min(), rtol=1e-9, atol=1e-15)
        if len(r) == 0:                                      # one entry: no return, no figures from them
            assert np.isnan(m[e, 2:5]).all()
            continue
        np.testing.assert_allclose(m[e, 2], r.mean(), rtol=1e-9, atol=1e-18)
        if len(r) < 2:
            assert np.isnan(m[e, 3]) and np.isnan(m[e, 4])
            continue
        np.testing.assert_allclose(m[e, 3], r.std(), rtol=1e-9, atol=1e-18)
        if flat[e]:                                          # zero variance: no Sharpe ratio
            assert m[e, 3] == 0 and np.isnan(m[e, 4]) and np.isnan(d["sharpe"][e])
        else:
            np.testing.assert_allclose(m[e, 4], 252 ** 0.5 * r.mean() / r.std(), rtol=1e-9)
            np.testing.assert_allclose(d["sharpe"][e], 2 * r.mean() / r.std(), rtol=1e-9)
    assert flat[length > 2].any()


# ------------------------------------------------------------------------------------------
# 6. a transactions slab past 4 GiB
# ------------------------------------------------------------------------------------------
def test_transactions_slab_past_4_gib():
    """65,536 envs x 32 assets: every entry of the f64 transactions slab is 16 MiB, entry 256 starts at
    byte 2^32.  A lock-step episode of 259 steps; the entries on both sides of the boundary against the
    audit rows read at those steps; early entries are still what they were (a wrapped offset would land
    there)."""
    _need_gpu()
    Panel, Env, _ = classes("cashpenalty")
    E, N, cap = 65_536, 32, 260
    need = cap * E * (N * 8 + 28) + (2 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of free device memory")
    close, info, turb = make_panel(N, 1, cap + 1)
    env = Env(Panel(close, info, turb), E, random_start=False, auto_reset=False, hmax=50.0, **COMMON)
    env.reset()
    hist = env.enable_history(actions=False)
    assert hist.capacity == cap + 1 and hist.tx.numel() * 8 > 2 ** 32 + 2 * E * N * 8
    assert 255 * E * N * 8 < 2 ** 32 == 256 * E * N * 8
    hist.tx.fill_(-7)
    rng = np.random.default_rng(61)
    pool = [_dev(rng.uniform(-1, 1, (E, N)).astype(np.float32)) for _ in range(4)]
    watch = (0, 1, 128, 254, 255, 256, 257, 258)
    snap = {}
    for k in range(cap - 1):                                 # entry k is written by the k-th step
        env.step(pool[k % 4])
        if k in watch:
            snap[k] = env.audit.clone()
    torch.cuda.synchronize()
    assert int(hist.length.min()) == int(hist.length.max()) == int(hist.ntx.min()) == cap - 1
    for k, au in snap.items():
        assert torch.equal(hist.tx[k], au[:, 4:]), k
        assert torch.equal(hist.cash[k], au[:, 0]) and torch.equal(hist.reward[k], au[:, 2]), k
        assert bool((au[:, 4:] != 0).any())
    assert bool((hist.tx[cap - 1:] == -7).all())             # nothing past the entries
