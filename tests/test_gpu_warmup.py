"""GPU: the warm-up kernels (csrc/adapt.hip behind `l2hmc_adapt_*`) against the float64 restatement of tests/warmup_case.py
after EVERY update of scripted sequences, their reproducibility, and `warmup` end to end on the library's own samplers.

Gates of the scripted sequences (set by reasoning, not by what the kernel gives), with the worst deviation measured on the
MI355X over all sequences beside each:

  mean accept                          relative 1e-10   float32 values summed in double: at most n 2^-53     measured 3.2e-16
  log_eps, log_eps_bar, H_bar, mu      absolute 1e-8    the update amplifies an error in `a` by at most
                                                        sqrt(30) / 0.05 ~ 110                                 measured 8.9e-15
  alpha                                within one float32 ulp of float32(log_eps)                             measured 0 ulp
  phase, dir, t, the counter           exact

End to end (fixtures L and G of tests/warmup_case.py, target 0.8, 100 updates of one proposal, two starting points): the mean
accept probability of 100 further proposals at the finished step size within 0.03 of the target, and the two finished step
sizes within a factor 1.05 of each other -- the caps tests/test_warmup_cpu.py first holds the restatement alone to."""
import math

import numpy as np
import pytest
import torch

from tests import warmup_case as wc

pytestmark = pytest.mark.gpu

BOUNDARY = 65536          # l2hmc_amd.warmup.SINGLE_BLOCK_MAX: one workgroup up to here, block partials + a second kernel beyond
# window sizes: the issue's list, the boundary's two sides, and the sizes at which the kernel's own loops change shape (1024
# threads, 8 loads per thread and round, chunks of 4096 values beyond the boundary, longer chunks beyond 4096 * 1024 values)
SIZES = [1, 63, 64, 65, 255, 256, 257, 4096, BOUNDARY, BOUNDARY + 1, 1023, 1024, 1025, 8191, 8192, 8193, BOUNDARY - 1,
         BOUNDARY + 4096, (1 << 20) + 3, 4096 * 1024 + 1025]
AVERAGING = [0.93, 0.41, 0.77, 0.85, 0.12, 0.99, 0.66, 0.8, 0.79, 0.31, 0.88, 0.72, 0.95, 0.05, 0.81, 0.83, 0.6, 0.74, 0.9, 0.22,
             0.86, 0.78, 0.69, 0.97, 0.35, 0.82, 0.84, 0.71, 0.58, 0.8]          # 30 averaging updates
# name -> (eps0, init keywords, scripted window means: search, then the crossing, then averaging)
SEQUENCES = {
    "up": (1e-3, {}, [0.99, 0.97, 0.9, 0.8, 0.62, 0.3] + AVERAGING),
    "down": (2.0, {}, [0.0, 0.05, 0.2, 0.41, 0.7] + AVERAGING[:6]),
    "cross_at_once_up": (0.1, {}, [0.9, 0.2] + AVERAGING[:4]),
    "cross_at_once_down": (0.1, {}, [0.2, 0.9] + AVERAGING[:4]),
    "clamp_binds_in_search": (0.3, {"eps_bounds": (1e-2, 1.0)}, [0.9, 0.9, 0.9] + AVERAGING[:8]),      # and clamps while averaging
    "clamp_binds_below": (0.03, {"eps_bounds": (1e-2, 1.0)}, [0.1, 0.1] + AVERAGING[:4]),
    "no_search": (0.25, {"search": False, "target_accept": 0.65, "gamma": 0.1, "t0": 5.0, "kappa": 0.6}, AVERAGING),
}
STATE_FLOATS, STATE_INTS = (3, 4, 5, 6), (0, 1, 2, 8)
_WORST = {"a": 0.0, "state": 0.0, "ulp": 0}


def _window(mean, n, rng):
    """n float32 accept probabilities around `mean`, with NaN, +inf and -inf entries (counted as 0) when there is room"""
    p = np.clip(mean + (0.1 if n >= 256 else 0.02) * rng.standard_normal(n), 0.0, 1.0).astype(np.float32)
    if n >= 63:
        p[rng.randint(0, n, 3)] = [np.nan, np.inf, -np.inf]
    elif n == 1 and mean < 0.2:
        p[0] = np.nan
    a = wc.window_mean(p)
    assert abs(a - 0.5) >= 1e-3, "a scripted mean too close to the branch"
    return p, a


def _ulps(a, b):
    ia, ib = (int(np.float32(v).view(np.int32)) for v in (a, b))
    ia, ib = (v if v >= 0 else -(v & 0x7fffffff) for v in (ia, ib))
    return abs(ia - ib)


def _compare(state, alpha, ref, where):
    got, want = state.cpu().numpy(), ref.state()
    for i in STATE_INTS:
        assert got[i] == want[i], (where, i, got[i], want[i])
    assert np.array_equal(got[9:], want[9:]), where
    e_a = abs(got[7] - want[7]) / max(abs(want[7]), 1e-300) if want[7] != 0 else abs(got[7])
    e_s = max(abs(got[i] - want[i]) for i in STATE_FLOATS)
    ulp = _ulps(alpha.item(), np.float32(want[3]))
    _WORST["a"], _WORST["state"], _WORST["ulp"] = max(_WORST["a"], e_a), max(_WORST["state"], e_s), max(_WORST["ulp"], ulp)
    assert e_a <= 1e-10, (where, e_a)
    assert e_s <= 1e-8, (where, e_s)
    assert ulp <= 1, (where, ulp)
    return got


def _init_kw(kw):
    k = dict(kw)
    out = {}
    if "eps_bounds" in k:
        out["log_eps_min"], out["log_eps_max"] = (math.log(b) for b in k.pop("eps_bounds"))
    if "target_accept" in k:
        out["target"] = k.pop("target_accept")
    out.update(k)
    return out


def _hmc(energy, d, eps):
    from l2hmc_amd import Dynamics
    return Dynamics(d, energy, T=wc.T, eps=eps, hmc=True)


def _gauss_energy(sd):
    from l2hmc_amd import distributions as D
    return D.Gaussian(np.zeros(len(sd)), np.diag(np.asarray(sd, dtype=np.float64) ** 2)).get_energy_function()


def _scripted(name, sizes_from=0):
    """run sequence `name` on the device, comparing with the restatement after every update; returns (state, alpha, trace rows)"""
    from l2hmc_amd.warmup import adapt_finish, adapt_init, adapt_update
    eps0, kw, means = SEQUENCES[name]
    dyn = _hmc(_gauss_energy([1.0, 2.0]), 2, eps0)
    alpha = dyn.alpha
    state = adapt_init(dyn, **kw)
    ref = wc.DualAveraging(float(alpha.item()), **_init_kw(kw))
    _compare(state, alpha, ref, (name, "init"))
    rng = np.random.RandomState(len(name))
    rows = torch.zeros((len(means) + 1, 4), dtype=torch.float64, device="cuda")
    for k, m in enumerate(means + [0.4]):
        if k == len(means):                       # finish, then one more update in phase 2
            adapt_finish(state, alpha)
            ref.finish()
            _compare(state, alpha, ref, (name, "finish"))
        n = SIZES[(sizes_from + k) % len(SIZES)]
        p, a = _window(m, n, rng)
        adapt_update(torch.as_tensor(p).cuda(), state, alpha, rows[k])
        want_row = ref.update(a)
        _compare(state, alpha, ref, (name, k, n))
        got_row = rows[k].cpu().numpy()
        assert got_row[3] == want_row[3] and abs(got_row[0] - want_row[0]) <= 1e-10 * max(want_row[0], 1e-300), (name, k)
        assert np.max(np.abs(got_row[1:3] - want_row[1:3])) <= 1e-8, (name, k)
    assert ref.phase == 2 and state[0].item() == 2.0
    return state.clone(), alpha.detach().clone(), rows


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_update_follows_the_restatement_after_every_update(name):
    # every sequence starts at another place of the size list; "up" (37 updates) walks it nearly twice
    _scripted(name, sizes_from=3 * sorted(SEQUENCES).index(name))
    print("%s: worst so far -- mean accept %.3g relative, state %.3g absolute, alpha %d ulp" % (
        name, _WORST["a"], _WORST["state"], _WORST["ulp"]))


def test_every_window_size_reduces_to_the_float64_mean():
    """mode REDUCE alone over the whole size list (both forms of the kernel, every loop shape): sums2 = {sum, n}"""
    from l2hmc_amd.warmup import REDUCE, adapt_update
    rng = np.random.RandomState(5)
    sums2 = torch.zeros(2, dtype=torch.float64, device="cuda")
    for n in SIZES:
        p, a = _window(0.7, n, rng)
        adapt_update(torch.as_tensor(p).cuda(), None, None, mode=REDUCE, sums2=sums2)
        s, cnt = sums2.cpu().numpy()
        assert cnt == n
        assert abs(s / cnt - a) <= 1e-10 * a, (n, s / cnt, a)


def test_same_sequence_twice_gives_identical_bits():
    s1, a1, r1 = _scripted("up")
    torch.empty(1 << 22, device="cuda").normal_()                  # other work, other addresses
    s2, a2, r2 = _scripted("up")
    assert torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32))
    assert torch.equal(r1.view(torch.int64), r2.view(torch.int64))


@pytest.mark.parametrize("n", [4096, 2 * BOUNDARY + 10])
def test_reduce_halves_then_apply_equals_one_launch(n):
    """what ranks do around one all-reduce: REDUCE on two halves, the sums added, APPLY -- against mode 3 on the whole window"""
    from l2hmc_amd.warmup import APPLY, REDUCE, adapt_init, adapt_update
    rng = np.random.RandomState(n)
    dyn_a, dyn_b = (_hmc(_gauss_energy([1.0, 2.0]), 2, 0.05) for _ in range(2))
    st_a, st_b = adapt_init(dyn_a), adapt_init(dyn_b)
    for m in [0.9, 0.8, 0.3] + AVERAGING[:5]:
        p = torch.as_tensor(_window(m, n, rng)[0]).cuda()
        adapt_update(p, st_a, dyn_a.alpha)
        h0, h1 = (torch.zeros(2, dtype=torch.float64, device="cuda") for _ in range(2))
        adapt_update(p[:n // 2 + 7], None, None, mode=REDUCE, sums2=h0)
        adapt_update(p[n // 2 + 7:], None, None, mode=REDUCE, sums2=h1)
        adapt_update(None, st_b, dyn_b.alpha, mode=APPLY, sums2=h0 + h1)
        a, b = st_a.cpu().numpy(), st_b.cpu().numpy()
        assert b[8] > 0 and all(a[i] == b[i] for i in STATE_INTS)
        assert np.max(np.abs(a - b)) <= 1e-10
    assert a[0] == 1 and a[2] == 5


def _dynamics(name, eps0):
    from l2hmc_amd import LogisticRegression
    f = wc.fixture(name)
    if name == "L":
        e = LogisticRegression(f["X"], f["y"], prior_var=1.0).get_energy_function()
    else:
        e = _gauss_energy(f["sd"])
    return _hmc(e, f["d"], eps0), torch.as_tensor(f["x0"]).cuda()


@pytest.mark.parametrize("name", ["L", "G"])
def test_end_to_end_meets_the_caps_and_repeats_bitwise(name):
    from l2hmc_amd import sample_chain, warmup
    eps, accepts = [], []
    for seed, e0 in enumerate(wc.EPS0[name]):
        dyn, x0 = _dynamics(name, e0)
        sample_chain(x0, dyn, 1, seed=0)                           # first launch: code objects, the packed data set
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                    # no synchronise, no device-to-host copy inside warmup
        try:
            x, info = warmup(x0, dyn, wc.N_UPDATES, target_accept=wc.TARGET, seed=seed + 1)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert info.next_proposal0 == wc.N_UPDATES and tuple(info.trace.shape) == (wc.N_UPDATES, 4)
        assert info.n_search + info.n_averaged == wc.N_UPDATES and info.n_averaged >= 50
        assert np.float32(info.log_eps) == dyn.alpha.item() and abs(info.eps - dyn.eps.item()) < 1e-6 * info.eps
        _, p, _ = sample_chain(x, dyn, wc.N_CHECK, seed=seed + 1, proposal0=info.next_proposal0)
        acc = float(p.double().mean())
        print("fixture %s from eps0 %g: eps %.4f, accept %.4f over %d further proposals, %d search + %d averaging updates" % (
            name, e0, info.eps, acc, wc.N_CHECK, info.n_search, info.n_averaged))
        eps.append(info.eps)
        accepts.append(acc)
        if seed == 0:                                              # the same call with the same seed: the same bits
            dyn2, _ = _dynamics(name, e0)
            x2, info2 = warmup(x0, dyn2, wc.N_UPDATES, target_accept=wc.TARGET, seed=seed + 1)
            assert torch.equal(dyn2.alpha.view(torch.int32), dyn.alpha.view(torch.int32))
            assert torch.equal(x2, x) and torch.equal(info2.state.view(torch.int64), info.state.view(torch.int64))
    assert all(abs(a - wc.TARGET) <= wc.CAP_ACCEPT for a in accepts), accepts
    ratio = eps[0] / eps[1]
    assert max(ratio, 1.0 / ratio) <= wc.CAP_RATIO, eps


def test_no_stale_step_size():
    """no prepared copy holds eps: the launch after a warm-up equals a fresh Dynamics built at the adapted float32 value"""
    from l2hmc_amd import sample_chain, warmup
    dyn, x0 = _dynamics("L", 1e-4)
    sample_chain(x0, dyn, 2, seed=3)                               # everything a launch prepares exists BEFORE the warm-up
    x, info = warmup(x0, dyn, 30, seed=4)
    a = sample_chain(x, dyn, 8, seed=5)
    fresh, _ = _dynamics("L", 1.0)
    fresh.alpha.copy_(dyn.alpha)
    assert fresh.alpha.item() == np.float32(info.log_eps) and info.eps > 1e-2
    b = sample_chain(x, fresh, 8, seed=5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_fused_nets_keep_their_parameters_and_the_trainer_sees_alpha():
    from l2hmc_amd import Dynamics, layers, sample_chain, warmup
    from l2hmc_amd.training import Trainer
    torch.manual_seed(0)
    np.random.seed(0)
    dyn = Dynamics(2, _gauss_energy([1.0, 0.3]), T=wc.T, eps=0.01, net_factory=layers.stq_network(10))
    trainer = Trainer(dyn)
    alpha, ptr = dyn.alpha, dyn.alpha.data_ptr()
    before = [(k, v.detach().clone()) for k, v in dyn.parameters() if k != "alpha"]
    x0 = torch.as_tensor(np.random.RandomState(1).randn(256, 2).astype(np.float32)).cuda()
    x, info = warmup(x0, dyn, 10, seed=2)
    assert dyn.alpha is alpha and isinstance(alpha, torch.nn.Parameter) and alpha.data_ptr() == ptr
    for (k, old), (k2, new) in zip(before, [(k, v) for k, v in dyn.parameters() if k != "alpha"]):
        assert k == k2 and torch.equal(old.view(torch.int32), new.detach().view(torch.int32)), k
    assert alpha.item() != np.float32(math.log(0.01)) and alpha.item() == np.float32(info.log_eps)
    assert trainer.theta[-1].item() == alpha.item()
    _, p, _ = sample_chain(x, dyn, 4, seed=3)
    assert torch.isfinite(p).all()


def test_slow_path_adapts_too():
    """a caller-supplied energy (torch callable, GEMM engine): the standard normal in d = 4, 64 chains, 12 updates from 1e-3"""
    from l2hmc_amd import Dynamics, warmup
    dyn = Dynamics(4, lambda x: 0.5 * (x * x).sum(1), T=wc.T, eps=1e-3, hmc=True)
    x0 = torch.as_tensor(np.random.RandomState(2).randn(64, 4).astype(np.float32)).cuda()
    x, info = warmup(x0, dyn, 12, seed=6)
    phases = info.trace[:, 3].cpu().numpy()
    assert info.eps > 0.05 and dyn.eps.item() > 0.05
    assert phases[0] == 0 and phases[-1] == 1 and np.all(np.diff(phases) >= 0) and info.n_search >= 1


def test_sharded_warmup_on_one_rank_equals_warmup_bitwise():
    from l2hmc_amd import sharding, warmup
    out = []
    for fn in (warmup, sharding.warmup):
        dyn, x0 = _dynamics("G", 1e-3)
        x, info = fn(x0, dyn, 25, seed=9, proposals_per_update=2)
        out.append((x, info.state, info.trace, dyn.alpha.detach()))
        assert info.next_proposal0 == 50
    for a, b in zip(*out):
        assert torch.equal(a, b)
