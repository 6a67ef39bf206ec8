"""Episode history of the batched stock env (VecStockTradingEnv.enable_history(),
finenv_stock_set_history) on the MI355X: the per-env asset_memory / date_memory / actions_memory the
record kernel keeps on the device must be the reference's -- the committed reference fixtures, the
reference's own frames and CSV texts, and the CPU oracle's series.  asset, row, actions, length and flags
are compared exactly everywhere (the series is the fp64 value the reference appends); mean / std /
Sharpe of metrics() against pandas keep the bound the project uses for that quantity across summation
orders (rtol 1e-9, atol 1e-12: _stats_equal of test_gpu_stock_windows.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from _golden import StockFixture, stock_fixture_names

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)

COMPLETE, OVERFLOW = 1, 2


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: GPU tests must run on the MI355X box")


def _random_panel(seed, T, N, K, flag_frac=0.03):
    rng = np.random.default_rng(seed)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.01, (T, N)), axis=0))
    tech = rng.normal(0, 1, (T, K, N))
    if K:
        tech[:, 0, :][rng.random((T, N)) < flag_frac] = 1.0
    risk = np.abs(rng.normal(0, 30, T))
    return close, tech, risk


def _host(hist, ids=None):
    """Host copy of a history (of the envs `ids`): one copy per tensor."""
    def pick(t, dim):
        if t is None:
            return None
        if ids is not None:
            t = t.index_select(dim, torch.as_tensor(np.asarray(ids), dtype=torch.int64, device=t.device))
        return t.cpu().numpy()
    return dict(asset=pick(hist.asset, 1), row=pick(hist.row, 1), actions=pick(hist.actions, 1),
                length=pick(hist.length, 0), flags=pick(hist.flags, 0))


def _clone(hist):
    return {k: getattr(hist, k).clone() for k in ("asset", "row", "actions", "length", "flags")
            if getattr(hist, k) is not None}


def _same(hist, snap):
    return all(torch.equal(getattr(hist, k), v) for k, v in snap.items())


# ------------------------------------------------------------------------------------------------
# 1. the reference fixtures: asset_memory / actions_memory of both episodes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", stock_fixture_names())
def test_history_equals_reference_fixture(name):
    """The fixture replayed as test_gpu_stock_parity.py replays it (gym semantics, host reset where the
    fixture resets) on 130 replicas -- two full waves and a partial one: after each of its two episodes
    the record is the reference's asset_memory and the `realised` rows of that episode."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    fx = StockFixture(name)
    z = fx.z
    E = 130
    env = VecStockTradingEnv(StockPanel(fx.close, fx.tech, fx.risk), E, auto_reset=False, **fx.env_kwargs())
    hist = env.enable_history()
    assert env.enable_history() is hist and hist.capacity == fx.T
    resets = z["reset_step"].tolist()
    if -1 in resets:
        env.reset()
    tj, ep_start = 0, 0
    for s in range(fx.S):
        a = torch.from_numpy(np.broadcast_to(fx.actions[s], (E, fx.N)).copy()).cuda()
        env.step(a)
        if not z["done"][s]:
            continue
        am = z[f"asset_memory_{tj}"]
        h = _host(hist)
        n = len(am)
        np.testing.assert_array_equal(h["length"], np.full(E, n), err_msg=f"episode {tj}")
        np.testing.assert_array_equal(h["flags"], np.full(E, COMPLETE))
        np.testing.assert_array_equal(h["asset"][:n], np.broadcast_to(am[:, None], (n, E)),
                                      err_msg=f"asset_memory_{tj}")
        np.testing.assert_array_equal(h["row"][:n], np.broadcast_to((fx.T - n + np.arange(n))[:, None], (n, E)))
        real = z["realised"][ep_start:s]
        assert len(real) == n - 1
        np.testing.assert_array_equal(h["actions"][:n - 1], np.broadcast_to(real[:, None, :], (n - 1, E, fx.N)),
                                      err_msg=f"actions_memory of episode {tj}")
        tj += 1
        ep_start = s + 1
        assert s in resets
        env.reset()
        assert int(hist.length.min()) == int(hist.length.max()) == 1 and int(hist.flags.abs().sum()) == 0
    assert tj == 2
    # the steps after the second reset are a record in progress
    h = _host(hist)
    np.testing.assert_array_equal(h["length"], np.full(E, 1 + fx.S - ep_start))
    np.testing.assert_array_equal(h["flags"], np.zeros(E, np.int32))


# ------------------------------------------------------------------------------------------------
# 2. DRL_prediction's frames
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sb3_stock", "sb3_stock_turb"])
def test_save_memory_frames_equal_the_reference(name):
    """The reference's DRL_prediction loop (scripted model) on 130 replicas of its env:
    save_asset_memory(e) / save_action_memory(e) equal the frames it returned -- values, dates, column
    names, index name."""
    _need_gpu()
    import harness_loops as hl
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    z = np.load(os.path.join(GOLDEN, f"harness_{name}.npz"), allow_pickle=False)
    T, N, K, hmax, use_t = z["cfg_int"].tolist()
    cash0, bc, sc, rs, thr = z["cfg_float"].tolist()
    panel = StockPanel(z["close"], z["tech"], z["risk"], dates=z["account_date"].tolist(),
                       tickers=z["action_columns"].tolist())
    E = 130
    env = VecStockTradingEnv(panel, E, hmax=hmax, initial_amount=cash0, num_stock_shares=[0] * N,
                             buy_cost_pct=bc, sell_cost_pct=sc, reward_scaling=rs,
                             turbulence_threshold=thr if use_t else None, auto_reset=False)
    with pytest.raises(Exception, match="enable_history"):
        env.save_asset_memory()
    env.enable_history()
    model = hl.ScriptedModel(z["base"], 1 + np.arange(N))
    obs = env.reset().clone()                # get_sb_env()
    env.reset()                              # DRL_prediction's own reset (:113)
    for i in range(T):
        a, _ = model.predict(obs[:1].cpu().numpy())
        obs, _, done, _ = env.step(torch.from_numpy(np.broadcast_to(a, (E, N)).copy()).cuda())
    assert bool(done.all()) and bool(env.history.complete.all())
    accts, acts = env.save_asset_memory(), env.save_action_memory()
    assert len(accts) == len(acts) == E
    for e in range(E):
        acct, act = accts[e], acts[e]
        assert acct.columns.tolist() == ["date", "account_value"]
        assert acct["date"].tolist() == z["account_date"].tolist()
        np.testing.assert_array_equal(acct["account_value"].to_numpy(np.float64), z["account_value"])
        np.testing.assert_array_equal(act.to_numpy(np.int64), z["actions"])
        assert act.index.tolist() == z["action_date"].tolist()
        assert act.columns.tolist() == z["action_columns"].tolist()
        assert str(act.index.name) == str(z["action_index_name"])
    one = env.history.save_asset_memory(E - 1)          # a single env: a frame, not a list
    assert one.equals(accts[E - 1]) and env.save_asset_memory(3)[0].equals(accts[3])
    assert env.history.save_action_memory(64).equals(acts[64])


# ------------------------------------------------------------------------------------------------
# 3. the ensemble's validation and trade windows in one batch, no host loop
# ------------------------------------------------------------------------------------------------
def _scripted_batch(base, steps, obs, N):
    """harness_loops.ScriptedModel.predict for a whole batch at once: env e is at model step steps[e]."""
    v = obs[:, 1:N + 1]
    sgn = np.sign(v - np.roll(v, -1, axis=1)).astype(np.float32)
    return (np.float32(0.75) * base[steps % len(base)] + np.float32(0.25) * sgn).astype(np.float32)


def _run_windows_recorded(panel, windows, offsets, base, n_envs, **kw):
    """test_gpu_stock_windows.py::_run_windows with the history instead of state_numpy(): env e runs
    window windows[e % W], driven by the scripted model from step offsets[e % W]; nothing but the
    observation (the model's input) leaves the device while stepping.  -> (env, hand-over states)"""
    from finrl_amd.vec_env import VecStockTradingEnv
    W, N = len(windows), panel.N
    s = np.array([windows[e % W][0] for e in range(n_envs)])
    t = np.array([windows[e % W][1] for e in range(n_envs)])
    env = VecStockTradingEnv(panel, n_envs, windows=(s, t), auto_reset=False, **kw)
    hist = env.enable_history()
    assert hist.capacity == int((t - s).max())
    steps = np.array([offsets[e % W] for e in range(n_envs)])
    base = np.asarray(base, np.float32)
    obs = env.reset().cpu().numpy()
    for i in range(int((t - s).max())):
        a = _scripted_batch(base, steps + i, obs, N)
        obs = env.step(torch.from_numpy(a).cuda())[0].cpu().numpy()
    # the terminal step leaves the state as it is (auto_reset=False): the state on the second-to-last
    # day is still there after the loop
    st = env.state_numpy()
    last = []
    for e in range(n_envs):
        row = st["price_day"][e]
        last.append([float(st["cash"][e])] + panel.close[row].tolist()
                    + st["shares"][e].astype(np.int64).tolist() + panel.tech[row].reshape(-1).tolist())
    return env, last


@pytest.mark.parametrize("name", ["ensemble", "ensemble_dow30"])
def test_ensemble_windows_recorded_in_one_batch(name):
    """The ensemble's validation window and first trade window in ONE batch (65 replicas each), the
    second trade window (initial=False, seeded with the first one's hand-over state) in a second one:
    account_value_frame(e).to_csv(index=False) is the file the reference's terminal branch wrote,
    validation_sharpe() is get_validation_sharpe's figure."""
    _need_gpu()
    from finrl_amd import StockPanel
    z = np.load(os.path.join(GOLDEN, f"harness_{name}.npz"), allow_pickle=False)
    T, N, K, Tv, Tr, hmax, use_t = z["cfg_int"].tolist()
    cash0, bc, sc, rs, thr = z["cfg_float"].tolist()
    panel = StockPanel(z["close"], z["tech"], z["risk"], dates=z["dates"].tolist())
    kw = dict(hmax=hmax, buy_cost_pct=bc, sell_cost_pct=sc, reward_scaling=rs,
              turbulence_threshold=(thr if use_t else None))
    E = 130
    env1, last1 = _run_windows_recorded(panel, [(0, Tv), (Tv, Tv + Tr)], [0, Tv], z["base"], E,
                                        initial_amount=cash0, num_stock_shares=[0] * N, initial=True, **kw)
    for e in range(1, E, 2):
        np.testing.assert_array_equal(np.asarray(last1[e], np.float64), z["last_state_1"])
    ls1 = z["last_state_1"]
    env2, last2 = _run_windows_recorded(panel, [(Tv + Tr, T)], [Tv + Tr], z["base"], E,
                                        initial_amount=ls1[0],
                                        num_stock_shares=[int(x) for x in ls1[N + 1:2 * N + 1]],
                                        initial=False, **kw)
    for e in range(E):
        np.testing.assert_array_equal(np.asarray(last2[e], np.float64), z["last_state_2"])
    csv = dict(zip(z["csv_names"].tolist(), z["csv_texts"].tolist()))
    for fn, env, env_ids in (("account_value_validation_A2C_63.csv", env1, list(range(0, E, 2))),
                             ("account_value_trade_ensemble_126.csv", env1, list(range(1, E, 2))),
                             ("account_value_trade_ensemble_189.csv", env2, list(range(E)))):
        assert bool(env.history.complete.all()) and not bool(env.history.overflow.any())
        frames = env.history.account_value_frame(env_ids)
        for e, df in zip(env_ids, frames):
            assert df.to_csv(index=False) == csv[fn], (fn, e)
    sharpe = env1.history.validation_sharpe()
    print("validation sharpe", sharpe[0], "reference", float(z["sharpe"]))
    np.testing.assert_allclose(sharpe[0::2], float(z["sharpe"]), rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# the recording rule restated on the host, fed by the oracle
# ------------------------------------------------------------------------------------------------
class _Tracker:
    """What the history of the envs `ids` must hold, from a StockOracle that runs the same envs (on
    panel rows row0 ..): per env the oracle's end_total_asset (column 1 of episode_stats()) after each
    non-terminal step of the recorded episode, its panel row, and WHICH steps' realised rows belong to
    the record."""

    def __init__(self, orc, ids, row0=0):
        self.orc, self.ids, self.row0 = orc, np.asarray(ids), row0
        n = len(self.ids)
        self.asset = [[] for _ in range(n)]
        self.row = [[] for _ in range(n)]
        self.steps = [[] for _ in range(n)]
        self.complete = np.zeros(n, bool)

    def arm(self, local=None):
        st, day = self.orc.episode_stats(), self.orc.state()["day"]
        for j in (range(len(self.ids)) if local is None else local):
            # at the start of an episode asset_memory[0], else the current total asset
            self.asset[j] = [st[j, 0] if day[j] == 0 else st[j, 1]]
            self.row[j] = [self.row0 + int(day[j])]
            self.steps[j] = []
            self.complete[j] = False

    def step(self, actions, t, auto_reset=True):
        a = actions[self.ids]
        done = self.orc.vec_step(a, want_obs=False)[2] if auto_reset else self.orc.step(a, want_obs=False)[2]
        st, day = self.orc.episode_stats(), self.orc.state()["day"]
        for j in range(len(self.ids)):
            if not self.asset[j] or self.complete[j]:
                continue
            if done[j]:
                self.complete[j] = True
            else:
                self.asset[j].append(st[j, 1])
                self.row[j].append(self.row0 + int(day[j]))
                self.steps[j].append(t)
        return done

    def reset_envs(self, local):
        from oracle.stock import lib, _p
        row = np.empty(self.orc.D)
        for j in local:
            lib().stock_oracle_reset_env(self.orc._h, C.c_int(int(j)), _p(row))
        self.arm(local)

    def check(self, hist, realised_log, what=""):
        """realised_log: the env's `realised` output of every step so far, [steps][E, N] device tensors."""
        h = _host(hist, self.ids)
        ids_t = torch.as_tensor(self.ids, dtype=torch.int64, device=hist.length.device)
        real = torch.stack([r.index_select(0, ids_t) for r in realised_log]).cpu().numpy() \
            if realised_log else None
        for j, e in enumerate(self.ids):
            n = len(self.asset[j])
            msg = f"{what} env {e}"
            assert h["length"][j] == n, (msg, h["length"][j], n)
            assert h["flags"][j] == (COMPLETE if self.complete[j] else 0), msg
            np.testing.assert_array_equal(h["asset"][:n, j], np.asarray(self.asset[j]), err_msg=msg)
            np.testing.assert_array_equal(h["row"][:n, j], np.asarray(self.row[j]), err_msg=msg)
            if n > 1:
                np.testing.assert_array_equal(h["actions"][:n - 1, j], real[self.steps[j], j], err_msg=msg)


# ------------------------------------------------------------------------------------------------
# 4. auto-reset keeps the first episode; reset(mask) and arm() start new records
# ------------------------------------------------------------------------------------------------
def test_first_episode_survives_auto_reset_and_reset_rearms():
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, T, N, K = 200, 40, 30, 3
    close, tech, risk = _random_panel(11, T, N, K)
    windows = [(0, 9), (5, 20), (12, 40), (30, 36)]
    W = len(windows)
    s = np.array([windows[e % W][0] for e in range(E)])
    t = np.array([windows[e % W][1] for e in range(E)])
    kw = dict(hmax=100, initial_amount=300_000, turbulence_threshold=50.0)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, windows=(s, t), auto_reset=True, **kw)
    hist = env.enable_history()
    assert hist.capacity == 28 and env.realised is not None
    trackers = []
    for w, (lo, hi) in enumerate(windows):
        ids = np.arange(w, E, W)
        orc = StockOracle(close[lo:hi], tech[lo:hi], risk[lo:hi], n_envs=len(ids), **kw)
        orc.reset()
        trackers.append(_Tracker(orc, ids, lo))
    env.reset()
    for tr in trackers:
        tr.arm()
    rng = np.random.default_rng(5)
    log = []

    def run(n):
        for _ in range(n):
            a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
            _, _, done, _ = env.step(torch.from_numpy(a).cuda())
            log.append(env.realised.clone())
            d = np.zeros(E, bool)
            for tr in trackers:
                d[tr.ids] = tr.step(a, len(log) - 1)
            np.testing.assert_array_equal(done.cpu().numpy().astype(bool), d)

    run(4)                                       # mid-episode for every window
    for tr in trackers:
        tr.check(hist, log, "first episode, in progress")
    run(31)                                      # well past every window's first episode end
    assert bool(hist.complete.all())
    for tr in trackers:
        assert tr.complete.all()
        tr.check(hist, log, "first episode")
        for j, e in enumerate(tr.ids):           # the whole window, once
            assert len(tr.asset[j]) == t[e] - s[e]
    snap = _clone(hist)
    run(7)
    assert _same(hist, snap), "a finished record changed under later steps"

    # reset(mask) re-arms exactly the masked envs; their next episode is recorded
    mask = rng.random(E) < 0.4
    env.reset(torch.from_numpy(mask.astype(np.uint8)).cuda())
    for tr in trackers:
        tr.reset_envs(np.nonzero(mask[tr.ids])[0])
    h = _host(hist)
    np.testing.assert_array_equal(h["length"][mask], 1)
    np.testing.assert_array_equal(h["flags"][mask], 0)
    np.testing.assert_array_equal(h["row"][0][mask], s[mask])
    np.testing.assert_array_equal(h["asset"][0][mask], env.state["asset0"].cpu().numpy()[mask])
    for k, v in snap.items():                    # the others keep their finished record
        keep = torch.from_numpy(~mask).cuda()
        dim = 0 if v.dim() == 1 else 1
        idx = torch.nonzero(keep)[:, 0]
        assert torch.equal(getattr(hist, k).index_select(dim, idx), v.index_select(dim, idx)), k
    run(30)
    for tr in trackers:
        tr.check(hist, log, "episode after reset(mask)")
    assert bool(hist.complete.all())

    # an explicit arm() mid-episode starts a record at the current total asset
    run(2)
    mask2 = rng.random(E) < 0.5
    day = env.state["day"].cpu().numpy()
    mid = mask2 & (day != env.state["start_day"].cpu().numpy())
    assert mid.sum() > 10
    hist.arm(torch.from_numpy(mask2).cuda())
    for tr in trackers:
        tr.arm(np.nonzero(mask2[tr.ids])[0])
    h = _host(hist)
    np.testing.assert_array_equal(h["asset"][0][mid], env.total_asset().cpu().numpy()[mid])
    np.testing.assert_array_equal(h["row"][0][mask2], day[mask2])
    run(3)
    for tr in trackers:
        tr.check(hist, log, "after arm(mask)")


# ------------------------------------------------------------------------------------------------
# 5. random batches against the oracle, every kernel width
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desync", [False, True])
@pytest.mark.parametrize("N", [1, 7, 30, 33, 64, 65, 100, 128])
def test_history_matches_oracle_random_batch(N, desync):
    """Distinct action streams per env, E not a multiple of 64, auto-reset; lock-step, and with the
    desynchronised-batch hint on a batch whose envs are spread over the days by masked resets (which
    re-arm them)."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    E, T, K = 150 + N, 12, 2
    close, tech, risk = _random_panel(N, T, N, K)
    rng = np.random.default_rng(100 + N)
    cash0 = 200_000 * rng.uniform(0.5, 1.5, E)
    sh0 = rng.integers(0, 15, (E, N))
    kw = dict(hmax=60, initial_amount=cash0, num_stock_shares=sh0, buy_cost_pct=0.0013,
              sell_cost_pct=0.0007, turbulence_threshold=45.0)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, auto_reset=True, **kw)
    env.hint_desynchronised(desync)
    hist = env.enable_history()
    orc = StockOracle(close, tech, risk, n_envs=E, **kw)
    tr = _Tracker(orc, np.arange(E))
    tr.arm()
    tr.check(hist, [], "armed by enable_history")      # the constructor's episode, before any reset
    env.reset()
    orc.reset()
    tr.arm()
    log = []
    for step in range(2 * T + 4):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        a[rng.random((E, N)) < 0.05] = 0.0
        env.step(torch.from_numpy(a).cuda())
        log.append(env.realised.clone())
        tr.step(a, step)
        if desync and step in (2, 5, 9, 16):
            m = rng.random(E) < 0.3
            env.reset(torch.from_numpy(m.astype(np.uint8)).cuda())
            tr.reset_envs(np.nonzero(m)[0])
        if step in (3, T + 1):
            tr.check(hist, log, f"step {step}")
    if desync:
        assert len(np.unique(env.state["day"].cpu().numpy())) > 1
    tr.check(hist, log, "end")
    assert tr.complete.sum() > E // 2


def test_history_of_a_batch_larger_than_one_round_of_blocks():
    """The batch of test_gpu_fullsize.py::test_batches_larger_than_one_round_of_blocks (N = 30): the
    step is several launches, the record kernel runs once behind the last; sampled envs (the round
    boundaries among them) against the oracle, whole-batch properties for the rest."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    from oracle.stock import StockOracle
    N, E, T, K = 30, 69_700, 9, 2
    rng = np.random.default_rng(N + E)
    close = 100 * np.exp(np.cumsum(rng.normal(0, 0.02, (T, N)), axis=0))
    tech = rng.normal(0, 1, (T, K, N))
    risk = np.abs(rng.normal(0, 30, T))
    kw = dict(hmax=40, initial_amount=60_000, turbulence_threshold=45.0)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    hist = env.enable_history()
    sample = np.unique(np.concatenate([[0, 63, 64, 255, 256, E - 1, E - 2, E // 2, E // 2 + 1],
                                       rng.choice(E, 250, replace=False)]))
    blocks = (E + 63) // 64
    for k in (2, 3):
        chunk = (blocks + k - 1) // k
        for b in range(chunk, blocks, chunk):
            sample = np.union1d(sample, [min(E - 1, 64 * b - 1), min(E - 1, 64 * b), min(E - 1, 64 * b + 63)])
    orc = StockOracle(close, tech, risk, n_envs=len(sample), **kw)
    tr = _Tracker(orc, np.arange(len(sample)))     # the oracle and the tracker see the sample only
    env.reset()
    orc.reset()
    tr.arm()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(E)
    log = []
    sample_t = torch.from_numpy(sample).cuda()
    for step in range(T + 3):
        a = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
        env.step(a)
        log.append(env.realised[sample_t].clone())
        tr.step(a[sample_t].cpu().numpy(), step)

    class _Sampled:                                # the history restricted to the sample
        asset, row = hist.asset[:, sample_t], hist.row[:, sample_t]
        actions = hist.actions[:, sample_t]
        length, flags = hist.length[sample_t], hist.flags[sample_t]
    tr.check(_Sampled, log, "sampled")
    # lock-step batch: every env holds the whole episode, finished, on the same rows
    assert bool((hist.length == T).all()) and bool((hist.flags == COMPLETE).all())
    assert bool((hist.row == torch.arange(T, device="cuda", dtype=torch.int32)[:, None]).all())
    assert bool(torch.isfinite(hist.asset).all()) and float(hist.asset.min()) > 0


# ------------------------------------------------------------------------------------------------
# 6. inside a captured graph
# ------------------------------------------------------------------------------------------------
def test_history_in_a_captured_graph_equals_eager():
    _need_gpu()
    import bench
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    close, tech, risk = bench.synth_panel()
    close, tech, risk = close[:20], tech[:20], risk[:20]
    E, N, n_steps = 2048 + 70, 30, 8
    envs = [VecStockTradingEnv(StockPanel(close, tech, risk), E, **bench.ENV_KW) for _ in range(2)]
    hists = [e.enable_history() for e in envs]            # attached before the capture
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4)
    acts = [torch.rand(E, N, generator=gen, device="cuda") * 2 - 1 for _ in range(n_steps)]
    for e in envs:
        e.reset()
    eager, graphed = envs
    # warm up on a side stream, then put state and record back where they were
    state0 = {k: v.clone() for k, v in graphed.state.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for a in acts[:2]:
            graphed.step(a)
    torch.cuda.current_stream().wait_stream(side)
    for k, v in graphed.state.items():
        v.copy_(state0[k])
    hists[1].arm()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for a in acts:
            graphed.step(a)
    for rep in range(3):                                  # 24 steps: across the episode end at 19
        for a in acts:
            eager.step(a)
        g.replay()
        for k in ("asset", "row", "actions", "length", "flags"):
            assert torch.equal(getattr(hists[0], k), getattr(hists[1], k)), (rep, k)
        for k in eager.state:
            assert torch.equal(eager.state[k], graphed.state[k]), (rep, k)
        assert torch.equal(eager.obs, graphed.obs)
        assert int(hists[0].length[0]) == min(1 + n_steps * (rep + 1), 20)
    assert bool(hists[1].complete.all())


def test_history_with_rollout_buffer_graphed_segment_and_sb3_adapter():
    """The consumers that hand step() their own output tensors keep working with a history attached:
    RolloutBuffer (step(out=...): `done` lives in the buffer's slice) eager and inside a GraphedSegment --
    built first, then arm(), the documented order -- give the same record and the same buffers; the SB3
    adapter's env records too."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.graph import GraphedSegment
    from finrl_amd.rollout import RolloutBuffer
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T, N, K, n_steps = 600, 14, 30, 3, 9
    close, tech, risk = _random_panel(17, T, N, K)
    kw = dict(hmax=100, initial_amount=400_000)
    envs = [VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw) for _ in range(2)]
    hists = [e.enable_history() for e in envs]
    w = torch.randn(envs[0].obs.shape[1], N, device="cuda") * 1e-5

    def policy(obs):
        a = torch.tanh(obs @ w)
        return a, a.sum(1), a.mean(1)

    bufs = [RolloutBuffer(n_steps, E, envs[0].obs.shape[1], N) for _ in range(2)]
    o0, o1 = envs[0].reset().clone(), envs[1].reset().clone()
    seg = GraphedSegment(envs[1], policy, bufs[1])
    hists[1].arm()                                       # the segment's warm-up steps were recorded
    for rep in range(2):                                 # 18 steps: across the episode end at 13
        last0 = bufs[0].collect(envs[0], policy, o0).clone()
        seg.replay(o1)
        for name in ("obs", "rewards", "dones"):
            assert torch.equal(getattr(bufs[0], name), getattr(bufs[1], name)), (rep, name)
        # entries at or past length[e] are unspecified (the graphed env's hold its warm-up's)
        assert torch.equal(hists[0].length, hists[1].length) and torch.equal(hists[0].flags, hists[1].flags)
        live = torch.arange(T, device="cuda")[:, None] < hists[0].length[None, :]
        for k in ("asset", "row"):
            z = torch.zeros((), dtype=getattr(hists[0], k).dtype, device="cuda")
            assert torch.equal(torch.where(live, getattr(hists[0], k), z),
                               torch.where(live, getattr(hists[1], k), z)), (rep, k)
        assert torch.equal(hists[0].actions * live[1:, :, None], hists[1].actions * live[1:, :, None]), rep
        o0, o1 = last0, bufs[1].obs[n_steps].clone()
    assert bool(hists[0].complete.all()) and int(hists[0].length.min()) == T
    # the record is the env's own end_total_asset series: its last entry is the latched end asset
    envs[0].enable_last_episode()
    vec = envs[0].as_sb3_vec_env()
    vec.reset()                                          # re-arms
    assert int(hists[0].length.max()) == 1 and not bool(hists[0].complete.any())
    for i in range(T):
        _, _, dones, infos = vec.step(np.zeros((E, N), np.float32) + 0.3)
    assert dones.all() and bool(hists[0].complete.all())
    end = np.array([i["episode_summary"]["end_total_asset"] for i in infos])
    np.testing.assert_array_equal(hists[0].asset[T - 1].cpu().numpy(), end)


# ------------------------------------------------------------------------------------------------
# 7. non-interference, capacity
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [30, 100])
def test_history_does_not_change_the_env(N):
    """The same seeded run with and without a history: bit-identical obs, reward, done, state and
    last-episode block."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T, K = 333, 11, 3
    close, tech, risk = _random_panel(2, T, N, K)
    kw = dict(hmax=100, initial_amount=250_000, turbulence_threshold=50.0)
    envs = [VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw) for _ in range(2)]
    for e in envs:
        e.enable_last_episode()
        e.enable_realised()
    envs[1].enable_history()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(N)
    assert torch.equal(envs[0].reset(), envs[1].reset())
    for s in range(3 * T):
        a = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
        outs = [e.step(a) for e in envs]
        for x, y in zip(outs[0][:3], outs[1][:3]):
            assert torch.equal(x, y), s
        assert torch.equal(envs[0].realised, envs[1].realised)
        if s == T + 2:
            m = (torch.rand(E, generator=gen, device="cuda") < 0.3).to(torch.uint8)
            assert torch.equal(envs[0].reset(m), envs[1].reset(m))
    for k in envs[0].state:
        assert torch.equal(envs[0].state[k], envs[1].state[k]), k
    assert torch.equal(torch.nan_to_num(envs[0]._last, nan=-1.0), torch.nan_to_num(envs[1]._last, nan=-1.0))
    assert torch.equal(torch.nan_to_num(envs[0].last_episode_stats(), nan=-1.0),
                       torch.nan_to_num(envs[1].last_episode_stats(), nan=-1.0))


@pytest.mark.parametrize("with_actions", [True, False])
def test_capacity_shorter_than_the_episode(with_actions):
    """A caller-owned history (through the C ABI, as a foreign binding would attach it) whose capacity is
    shorter than the episode, each tensor followed by sentinel rows: the entries below the capacity equal
    those of a full-size history, the overflow flag is set, the sentinels are intact."""
    _need_gpu()
    from finrl_amd import StockPanel
    from finrl_amd import _native as nat
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T, N, K, cap, pad = 130, 14, 30, 2, 6, 3
    close, tech, risk = _random_panel(8, T, N, K)
    kw = dict(hmax=100, initial_amount=250_000, auto_reset=False)
    full_env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    full = full_env.enable_history(actions=with_actions)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, **kw)
    if with_actions:
        env.enable_realised()
    SENT_F, SENT_I = -12345.5, -777
    asset = torch.full((cap + pad, E), SENT_F, dtype=torch.float64, device="cuda")
    row = torch.full((cap + pad, E), SENT_I, dtype=torch.int32, device="cuda")
    actions = torch.full((cap - 1 + pad, E, N), SENT_I, dtype=torch.int32, device="cuda")
    length = torch.zeros(E + 64, dtype=torch.int32, device="cuda")
    flags = torch.zeros(E + 64, dtype=torch.int32, device="cuda")
    length[E:] = SENT_I
    flags[E:] = SENT_I
    ptrs = nat.StockHistoryPtrs(asset.data_ptr(), row.data_ptr(),
                                actions.data_ptr() if with_actions else None,
                                length.data_ptr(), flags.data_ptr(), cap)
    env._call("set_history", C.byref(ptrs))
    # attached, not armed: nothing is recorded
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    a0 = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
    env.step(a0)
    full_env.step(a0)
    assert int(length[:E].abs().sum()) == 0 and bool((asset == SENT_F).all()) and bool((row == SENT_I).all())
    env.reset()                                   # arms
    full_env.reset()
    for s in range(T - 1):
        a = torch.rand(E, N, generator=gen, device="cuda") * 2 - 1
        env.step(a)
        full_env.step(a)
        want = OVERFLOW if s + 1 >= cap else 0
        if s in (cap - 2, cap - 1, cap):
            assert bool((flags[:E] == want).all()), s
    _, _, done, _ = env.step(a0)
    full_env.step(a0)
    assert bool(done.all())
    assert bool((full.length == T).all()) and bool((full.flags == COMPLETE).all())
    assert bool((length[:E] == cap).all()) and bool((flags[:E] == (COMPLETE | OVERFLOW)).all())
    assert torch.equal(asset[:cap], full.asset[:cap]) and torch.equal(row[:cap], full.row[:cap])
    assert bool((asset[cap:] == SENT_F).all()) and bool((row[cap:] == SENT_I).all())
    assert bool((length[E:] == SENT_I).all()) and bool((flags[E:] == SENT_I).all())
    if with_actions:
        assert torch.equal(actions[:cap - 1], full.actions[:cap - 1])
        assert bool((actions[cap - 1:] == SENT_I).all())
    else:
        assert bool((actions == SENT_I).all()) and full.actions is None
    env._call("set_history", None)                # detach before the tensors go away


# ------------------------------------------------------------------------------------------------
# 8. metrics
# ------------------------------------------------------------------------------------------------
def test_metrics_against_pandas_and_the_last_episode_block():
    """metrics() against pandas on the recorded series copied to the host; n_returns, cumulative_return
    and max_drawdown exactly, mean / std / Sharpe within rtol 1e-9, atol 1e-12.  Envs are spread over
    windows of 2 .. 30 rows (one return, hence no std, up to 29), a sixth of them trade nothing (constant
    series: std == 0), some are unarmed.  metrics(252 ** 0.5)'s Sharpe against last_episode_stats()."""
    _need_gpu()
    import pandas as pd
    from finrl_amd import StockPanel
    from finrl_amd.vec_env import VecStockTradingEnv
    E, T, N, K = 300, 40, 30, 2
    close, tech, risk = _random_panel(21, T, N, K)
    rng = np.random.default_rng(3)
    length = rng.integers(2, 31, E)
    length[:4] = (2, 3, 30, 30)
    s = rng.integers(0, T - length + 1)
    env = VecStockTradingEnv(StockPanel(close, tech, risk), E, windows=(s, s + length), hmax=100,
                             initial_amount=500_000, auto_reset=False)
    env.enable_last_episode()
    hist = env.enable_history(actions=False)
    assert hist.actions is None and hist.capacity == 30
    idle = (np.arange(E) % 6 == 5)
    env.reset()
    for i in range(33):
        a = rng.uniform(-1, 1, (E, N)).astype(np.float32)
        a[idle] = 0.0
        env.step(torch.from_numpy(a).cuda())
    assert bool(hist.complete.all())
    unarmed = np.arange(E) % 50 == 7
    hist.length[torch.from_numpy(unarmed).cuda()] = 0
    h = _host(hist)
    from finrl_amd.history import METRIC_KEYS
    assert METRIC_KEYS == ("n_returns", "cumulative_return", "mean", "std", "sharpe", "max_drawdown")
    for ann in (252 ** 0.5, 4 ** 0.5):
        m = hist.metrics(ann).cpu().numpy()
        assert m.shape == (E, 6)
        worst = 0.0
        for e in range(E):
            n = h["length"][e]
            if n == 0:
                assert np.isnan(m[e]).all(), e
                continue
            assert n == length[e]
            ser = pd.Series(h["asset"][:n, e])
            r = ser.pct_change(1)
            assert m[e, 0] == n - 1
            assert m[e, 1] == ser.iloc[-1] / ser.iloc[0] - 1, e
            assert m[e, 5] == (ser / ser.cummax() - 1).min(), e
            np.testing.assert_allclose(m[e, 2], r.mean(), rtol=1e-9, atol=1e-12, err_msg=f"mean {e}")
            std = r.std()
            np.testing.assert_allclose(m[e, 3], std, rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=f"std {e}")
            if n - 1 < 2 or std == 0:
                assert np.isnan(m[e, 4]), e
            else:
                ref = ann * r.mean() / std
                np.testing.assert_allclose(m[e, 4], ref, rtol=1e-9, atol=1e-12, err_msg=f"sharpe {e}")
                worst = max(worst, abs(m[e, 4] - ref) / abs(ref))
        print(f"annualization {ann:.4f}: worst relative Sharpe difference to pandas {worst:.3g}")
    assert np.isnan(m[0, 3]) and np.isnan(m[0, 4]) and m[0, 0] == 1         # one return: no std
    flat = idle & ~unarmed & (length > 2)
    assert flat.sum() > 10 and (m[flat, 3] == 0).all() and np.isnan(m[flat, 4]).all()
    vs = hist.validation_sharpe()
    assert (vs[flat] == 0.0).all()                # variance 0, mean 0 -> 0.0
    # the terminal printout's Sharpe, by two routes
    m = hist.metrics(252 ** 0.5).cpu().numpy()
    last = env.last_episode_stats().cpu().numpy()
    ok = ~unarmed
    np.testing.assert_allclose(m[ok, 4], last[ok, 5], rtol=1e-9, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(m[ok, 0], env.last_episode["ret_n"].cpu().numpy()[ok])
