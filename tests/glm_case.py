"""Shared by tests/test_glm_cpu.py, tests/test_gpu_glm.py, tests/test_gpu_glm_geometries.py and tools/glm_accuracy.py: seeded
inputs of the Poisson regression's model criticism (`l2hmc_amd.PoissonRegression`, l2hmc_amd/glm.py, csrc/glm.hip), a float64
restatement written from the definition with scipy's gammaln (independent of l2hmc_amd/glm.py) and the bounds of the device
path, derived from the inputs; at the end the rows on the edges of the float32 likelihood (`edge_case`, `nan_case`) and the
three entries called straight with poisoned, guarded outputs (`device_raw_glm`, `check_raw`).

Definitions, for draws W (S, d), rows X (n, d), counts y, offsets o (all float32 inputs, restated in float64):
    h = x_i . w_s + o_i    mu = exp(h)    ll = y_i h - mu - gammaln(y_i + 1)

The device bound, with eps = 2^-24 and A_si = sum_k |w_sk| |x_ik|: the float32 contraction is within (d + 8) eps A of the exact
eta (tests/predictive_case.py) and the sum h = eta + o adds one rounding, dh = (d + 8) eps A + eps |h|.  ll moves with h by
y dh + mu (e^dh - 1) <= (y + mu e^dh) dh, and the four float32 roundings of the device function (the product h log2 e and the
hardware exp2 inside mu: mu (|h| + 2) eps; the fused y h - mu: (y |h| + mu) eps; g rounded once: g eps; the last difference:
|ll| eps) stay inside 4 eps (y |h| + mu (2 + |h|) + g + |ll|):
    |d ll| <= (y + mu e^dh) dh + 4 eps (y |h| + mu (2 + |h|) + g + |ll|) = B_si
and the predictive mean alone: |d mu| <= mu e^dh dh + 4 eps mu (2 + |h|) = Bmu_si.  Per row, as tests/predictive_case.py
derives them with this B in the place of its own:
    |d mean mu| <= mean_s Bmu      |d lppd_i| <= max_s B      |d mean ll| <= mean_s B
    |d p_waic_i| <= (2 sd_i max_s B + (max_s B)^2) S / (S - 1) + 4 S 2^-52 mean_s ll^2

The finished numbers of PSIS-LOO are gated at K delta_i, delta_i = max_s B_si (order statistics are 1-Lipschitz in the sup
norm), with the sensitivities K below measured from the float64 route alone (`sensitivity`, run by tools/glm_accuracy.py on the
CPU, times 4: sampled sign patterns under-estimate the worst case); profiles/glm_accuracy.txt records the run."""
import numpy as np

EPS = 2.0 ** -24

# (S, n, d): all four geometries (d = 1, 2, 3 -> 1 feature tile; 17 -> 2; 50 -> 4; 128 -> 8), rows past one workgroup's 32, a
# ragged last data block, a last draw tile that is not full, one, two and many chunks (several quads at S = 4099); and, with
# (70, 35, d), every count of live feature tiles NT = ceil(d / 16) that is below the compiled NTM -- the masks `tg < NT` of
# block_fragments and tile_logits, the label offset 512 NT, the zeroed LDS columns and tile_load's `e < tile_elems`
# (csrc/draw_tiles.hpp): d = 33 and 40 -> NT 3 / NTM 4; 65 -> 5 / 8 with one live column in the last tile; 96 -> 6 / 8 and
# 112 -> 7 / 8 with a full last tile; 100 -> 7 / 8 with a ragged one.  (d = 48 is not used: its mcse sensitivity, 79.2,
# lies above the recorded worst.)
SHAPES = [(25, 1, 1), (25, 3, 2), (70, 17, 3), (70, 33, 17), (70, 65, 50), (70, 50, 128), (4099, 100, 25),
          (70, 35, 33), (70, 35, 40), (70, 35, 65), (70, 35, 96), (70, 35, 100), (70, 35, 112)]
EXACT_SHAPES = [(70, 33, 3), (4099, 40, 3)]
AR1 = (200, 20, 3, 0.7, 63, False, 37)          # steps, chains, d, rho, max_lag, split, rows

# worst |change| / delta_i of the float64 route under +-B_si perturbations of ll, 8 seeded sign patterns, times 4
# (tools/glm_accuracy.py; profiles/glm_accuracy.txt)
# (the draws of `case` lie close together -- 0.1 randn about w0 -- so a row's ll spread is small against its level and the
# fitted shape moves a lot per unit of ll: the khat and mcse sensitivities are two orders above the logistic fixtures')
K_KHAT = 4 * 635        # worst measured 635, on (70, 33, 17)
K_ELPD = 4 * 2.8        # worst measured 2.78, on (25, 3, 2)
K_NEFF = 4 * 4.6        # relative; worst measured 4.53, on (25, 3, 2)
K_MCSE = 4 * 79         # relative; worst measured 78.2, on (70, 33, 17)
K_REFF = 4 * 22         # relative, on the AR(1) history; worst measured 21.2


def seed_of(S, n, d):
    return 9000 + S + n + d


def case(S, n, d, seed=None):
    """(W (S, d), X (n, d), y (n,), o (n,)) float32: X = randn, draws w0 + 0.1 randn scaled so that max |x . w| = 3, offsets
    uniform in [-1, 2], y ~ Poisson(exp(X w_mean + o)), and ONE surprising last row with y = ceil(3 mu + 5)."""
    rng = np.random.RandomState(seed_of(S, n, d) if seed is None else seed)
    X = rng.randn(n, d)
    W = rng.randn(d) + 0.1 * rng.randn(S, d)
    W *= 3.0 / np.abs(W @ X.T).max()
    o = rng.uniform(-1.0, 2.0, size=n)
    mu = np.exp(X @ W.mean(axis=0) + o)
    y = rng.poisson(mu).astype(np.float64)
    y[-1] = np.ceil(3.0 * mu[-1] + 5.0)
    return W.astype(np.float32), X.astype(np.float32), y.astype(np.float32), o.astype(np.float32)


def exact_case(S, n, d, seed):
    """Small-integer W with dyadic X and offsets: eta and h are exact in float32 and take few values, so ll has many ties."""
    rng = np.random.RandomState(seed)
    W = rng.randint(-1, 2, size=(S, d)).astype(np.float32)
    X = (rng.randint(-2, 3, size=(n, d)) / 4.0).astype(np.float32)
    o = (rng.randint(-4, 9, size=n) / 4.0).astype(np.float32)
    y = rng.poisson(np.exp(o.astype(np.float64))).astype(np.float32)
    return W, X, y, o


def ar1_case():
    """(W (M, N, d), X, y, o) float32: every chain an AR(1) series about a common offset, scaled like `case`."""
    M, N, d, rho, _, _, n = AR1
    rng = np.random.RandomState(9100)
    X = rng.randn(n, d)
    eps = rng.randn(M, N, d)
    Z = np.empty((M, N, d))
    Z[0] = eps[0]
    for t in range(1, M):
        Z[t] = rho * Z[t - 1] + np.sqrt(1.0 - rho * rho) * eps[t]
    W = rng.randn(d) + 0.1 * Z
    W *= 3.0 / np.abs(W.reshape(-1, d) @ X.T).max()
    o = rng.uniform(-1.0, 2.0, size=n)
    y = rng.poisson(np.exp(X @ W.reshape(-1, d).mean(axis=0) + o)).astype(np.float64)
    return W.astype(np.float32), X.astype(np.float32), y.astype(np.float32), o.astype(np.float32)


def log_lik(W, X, y, o):
    """(ll, h) float64 (S, n) from the definition."""
    from scipy.special import gammaln
    W, X, y, o = (np.asarray(a, dtype=np.float64) for a in (W, X, y, o))
    h = W.reshape(-1, X.shape[1]) @ X.T + o
    return y * h - np.exp(h) - gammaln(y + 1.0), h


def bounds(W, X, y, o):
    """{'B', 'Bmu' (S, n), 'delta' (n,), 'mean_mu', 'lppd_i', 'mean_ll', 'p_waic_i' (n,)} of the module docstring."""
    from scipy.special import gammaln
    ll, h = log_lik(W, X, y, o)
    S, d = ll.shape[0], X.shape[1]
    W64, X64, y64 = (np.asarray(a, dtype=np.float64) for a in (W, X, y))
    A = np.abs(W64.reshape(-1, d)) @ np.abs(X64).T
    dh = (d + 8) * EPS * A + EPS * np.abs(h)
    mu, g = np.exp(h), gammaln(y64 + 1.0)
    Bmu = mu * np.exp(dh) * dh + 4 * EPS * mu * (2 + np.abs(h))
    B = (y64 + mu * np.exp(dh)) * dh + 4 * EPS * (y64 * np.abs(h) + mu * (2 + np.abs(h)) + g + np.abs(ll))
    Bmax, sd = B.max(axis=0), ll.std(axis=0)
    return {"B": B, "Bmu": Bmu, "delta": Bmax, "mean_mu": Bmu.mean(axis=0), "lppd_i": Bmax, "mean_ll": B.mean(axis=0),
            "p_waic_i": (2 * sd * Bmax + Bmax ** 2) * S / (S - 1) + 4 * S * 2.0 ** -52 * (ll * ll).mean(axis=0)}


def restatement(W, X, y, o):
    """The predictive numbers per row, float64, from the definitions."""
    from scipy.special import logsumexp
    ll, h = log_lik(W, X, y, o)
    S = ll.shape[0]
    out = {"mean_mu": np.exp(h).mean(axis=0), "lppd_i": logsumexp(ll, axis=0) - np.log(S), "p_waic_i": ll.var(axis=0, ddof=1),
           "mean_ll": ll.mean(axis=0)}
    out["elpd_i"] = out["lppd_i"] - out["p_waic_i"]
    return out


def rel(a, b):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)


def sensitivity(S, n, d, patterns=8):
    """(K_khat, K_elpd, K_neff, K_mcse) of one shape: the worst |change| / delta_i of the float64 route
    (`psis.loo_from_log_lik` on the float64 matrix, with `loglik_case.r_eff_for(n)`) when ll moves by +-B_si."""
    from l2hmc_amd import psis
    from tests import loglik_case as lk
    W, X, y, o = case(S, n, d)
    ll, _ = log_lik(W, X, y, o)
    b = bounds(W, X, y, o)
    r = lk.r_eff_for(n)
    ref = psis.loo_from_log_lik(ll, r_eff=r)
    fin = np.isfinite(ref.khat)
    worst = np.zeros(4)
    rng = np.random.RandomState(77)
    for _ in range(patterns):
        got = psis.loo_from_log_lik(ll + np.where(rng.rand(*ll.shape) < 0.5, -1.0, 1.0) * b["B"], r_eff=r)
        both = fin & np.isfinite(got.khat)
        with np.errstate(all="ignore"):
            k = np.max((np.abs(got.khat - ref.khat) / b["delta"])[both]) if both.any() else 0.0
            vals = (k, np.max(np.abs(got.elpd_loo_i - ref.elpd_loo_i) / b["delta"]),
                    np.max((rel(got.n_eff, ref.n_eff) / b["delta"])[both]) if both.any() else 0.0,
                    np.max((rel(got.mcse_elpd_loo_i, ref.mcse_elpd_loo_i) / b["delta"])[both]) if both.any() else 0.0)
        worst = np.maximum(worst, vals)
    return tuple(float(v) for v in worst)


def reff_sensitivity(patterns=8):
    """The worst |relative change of r_eff| / delta_i of the float64 route on the AR(1) history when ll moves by +-B_si."""
    from l2hmc_amd import psis
    M, N, d, rho, max_lag, split, n = AR1
    W, X, y, o = ar1_case()
    ll, _ = log_lik(W, X, y, o)
    b = bounds(W, X, y, o)
    ref = psis.relative_eff_from_log_lik(ll.reshape(M, N, n), max_lag=max_lag, split=split)
    worst, rng = 0.0, np.random.RandomState(78)
    for _ in range(patterns):
        moved = ll + np.where(rng.rand(*ll.shape) < 0.5, -1.0, 1.0) * b["B"]
        got = psis.relative_eff_from_log_lik(moved.reshape(M, N, n), max_lag=max_lag, split=split)
        worst = max(worst, float(np.max(rel(got.r_eff, ref.r_eff) / b["delta"])))
    return worst


# ---- the edges of the likelihood ----------------------------------------------------------------------------------------------
MU_OVERFLOW_H = 88.7228       # float32 mu = exp2(h log2 e) is +inf from here on (h log2 e rounds to 128), so ll = -inf
EDGE_S = (70, 4099)
EDGE_ROWS = {"overflow_few": 0, "zero": 5, "underflow": 17, "overflow_many": 33, "large": 34}
EDGE_N = 37                   # rows 32 .. 36 are a ragged third data block in a second row group; its last row is ordinary


def tail_len(S):
    """M = min(S // 5, ceil(3 sqrt S)), the tail length of PSIS, restated."""
    return min(S // 5, int(np.ceil(3.0 * np.sqrt(S))))


def edge_case(S):
    """(W (S, 3), X (37, 3), y, o, ordinary) float32: the draws of `case(S, 32, 3)` and its 32 ordinary rows, in their order, at
    the indices `ordinary` (37,) bool; at `EDGE_ROWS` stand five rows on the edges of the float32 likelihood:
        overflow_few   between 1 and M - 1 draws have h > 88.8 (mu = +inf, ll = -inf): the tail holds -inf under a finite cutoff
        overflow_many  more than M draws have: the cutoff is -inf and the tail is empty
        zero           y = 0, offset -120: mu flushes to 0 and every ll is -0.0 -- a constant row, ties in the key order
        underflow      y = 300 at h about -3: ll - sat < -745 in every draw, so sum_lik = 0 and lppd_i = -inf
        large          y = 100000 at h about log y: y h and g cancel to eleven digits
    The two overflow rows are x = c u with u orthogonal to the mean draw and c so large that h spreads over the draws with a
    standard deviation of 40 at least (some draws keep exp(ll - sat) > 0: these rows do not count as underflowed) and that the
    widest gap between consecutive h in the wanted range of ranks is 0.3 at least; the offset puts the threshold inside that
    gap so that no draw's float64 h lies within 0.05 of it (tests/test_glm_cpu.py asserts all of this on the float64 h)."""
    W, X0, y0, o0 = case(S, 32, 3)
    rng = np.random.RandomState(9200 + S)
    W64 = W.astype(np.float64)
    wm = W64.mean(axis=0)
    M = tail_len(S)

    def spread(k_lo, k_hi):
        u = rng.randn(3)
        u -= (u @ wm) / (wm @ wm) * wm
        e = np.sort(W64 @ u)[::-1]
        gaps = e[k_lo - 1:k_hi] - e[k_lo:k_hi + 1]           # gaps[j]: k_lo + j draws lie above it
        x = (max(40.0 / e.std(), 0.3 / gaps.max()) * u).astype(np.float32)
        e = np.sort(W64 @ x.astype(np.float64))[::-1]
        k = k_lo + int(np.argmax(e[k_lo - 1:k_hi] - e[k_lo:k_hi + 1]))
        gap = e[k - 1] - e[k]
        return x, 88.8 + (gap - (88.8 - MU_OVERFLOW_H + 0.05)) / 2 - e[k - 1]

    def level(width, centre):
        x = rng.randn(3)
        e = W64 @ x
        x = (x * width / np.abs(e - e.mean()).max()).astype(np.float32)
        return x, centre - (W64 @ x.astype(np.float64)).mean()

    rows = {"overflow_few": spread(1, M - 1) + (2.0,), "overflow_many": spread(M + 1, S // 2) + (3.0,),
            "zero": (rng.randn(3).astype(np.float32), -120.0, 0.0), "underflow": level(0.5, -3.0) + (300.0,),
            "large": level(0.005, np.log(100000.0)) + (100000.0,)}
    X, y, o = np.zeros((EDGE_N, 3), dtype=np.float32), np.zeros(EDGE_N, dtype=np.float32), np.zeros(EDGE_N, dtype=np.float32)
    ordinary = np.ones(EDGE_N, dtype=bool)
    ordinary[list(EDGE_ROWS.values())] = False
    X[ordinary], y[ordinary], o[ordinary] = X0, y0, o0
    for name, i in EDGE_ROWS.items():
        X[i], o[i], y[i] = rows[name]
    return W, X, y, o, ordinary


def nan_case():
    """(W, X, y, o, W_bad): `case(4099, 35, 17)` and its draws with ONE NaN, in coordinate 5 of draw 1234."""
    W, X, y, o = case(4099, 35, 17)
    bad = W.copy()
    bad[1234, 5] = np.nan
    return W, X, y, o, bad


# ---- the device entries, straight (need a GPU) ---------------------------------------------------------------------------------
GUARD = 8                     # elements past the end of every output of `device_raw_glm`; they keep the fill


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    """Equal bit for bit, NaNs compared as NaNs, by position (a NaN's payload is no part of any contract here)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan]))


def device_raw_glm(data, W, lens=None, rows=None):
    """`l2hmc_glm_log_lik`, `l2hmc_glm_loo_tails` and `l2hmc_glm_predict` straight through `_ffi` on rows `rows` = (first, stop)
    (None: all) of the model data (X, y, o) under the draws W (numpy or a device tensor).  Every output is filled with NaN
    (floats) or -7 (integers) before the call and is GUARD elements longer than the entry is told, so that an element the
    kernel does not write shows and a write past the end shows as a changed guard, not as a fault:
    {'ll' (S, m), 'cutoff', 'top', 'n_tail' (m,), 'tail' (m, stride), 'sums' (3, m), 'psums' (4, m), 'flag', 'guards': name ->
    the GUARD trailing elements} numpy."""
    import torch
    from l2hmc_amd import _ffi, glm
    from l2hmc_amd._history import in_place, launch, workspace
    X, y, o = data
    Wd = in_place(W if hasattr(W, "is_cuda") else torch.as_tensor(np.ascontiguousarray(W, dtype=np.float32)).cuda())
    S, d = int(Wd.shape[0]), int(Wd.shape[1])
    a, stop = (0, X.shape[0]) if rows is None else rows
    m = stop - a
    dev, L = Wd.device, _ffi.lib()
    model = glm.Glm(np.ascontiguousarray(X, dtype=np.float32), np.ascontiguousarray(y, dtype=np.float32),
                    np.ascontiguousarray(o, dtype=np.float32))
    packed, consts = model._device_data(dev)(a, m)
    group = None if lens is None else np.ascontiguousarray(lens[a:stop], dtype=np.int64)
    stride = tail_len(S) if group is None else int(group.max())
    lens_d = None if group is None else torch.as_tensor(group).to(dev)

    def out(count, dtype):
        return torch.full((count + GUARD,), -7 if dtype == torch.int64 else float("nan"), dtype=dtype, device=dev)
    buf = {"ll": out(S * m, torch.float32), "cutoff": out(m, torch.float32), "top": out(m, torch.float32),
           "n_tail": out(m, torch.int64), "tail": out(m * stride, torch.float32), "sums": out(3 * m, torch.float64),
           "psums": out(4 * m, torch.float64)}
    fam = model.family
    launch(dev, L.l2hmc_glm_log_lik, Wd.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), m, fam, buf["ll"].data_ptr())
    ws = workspace(dev, torch.uint8, L.l2hmc_glm_loo_workspace_bytes, S, m, d)
    launch(dev, L.l2hmc_glm_loo_tails, Wd.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), m, fam,
           None if lens_d is None else lens_d.data_ptr(), stride, buf["cutoff"].data_ptr(), buf["top"].data_ptr(),
           buf["n_tail"].data_ptr(), buf["tail"].data_ptr() if stride else None, buf["sums"].data_ptr(), ws.data_ptr())
    wp = workspace(dev, torch.float64, L.l2hmc_glm_predict_workspace_doubles, S, m, d)
    launch(dev, L.l2hmc_glm_predict, Wd.data_ptr(), S, d, packed.data_ptr(), consts.data_ptr(), m, fam, buf["psums"].data_ptr(),
           wp.data_ptr())
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    shapes = {"ll": (S, m), "cutoff": (m,), "top": (m,), "n_tail": (m,), "tail": (m, stride), "sums": (3, m), "psums": (4, m)}
    res = {k: host[k][:-GUARD].reshape(shapes[k]) for k in host}
    res["guards"] = {k: host[k][-GUARD:] for k in host}
    res["flag"] = np.array([int(ws[:8].view(torch.int64)[0])])
    return res


def guards_untouched(res):
    """Every guard element of `device_raw_glm`'s result still holds its fill."""
    return all(np.all(g == -7) if g.dtype.kind == "i" else np.all(np.isnan(g)) for g in res["guards"].values())


def all_written(res):
    """No in-range element of `device_raw_glm`'s result holds its fill (for inputs whose outputs hold no NaN)."""
    return all(np.all(res[k] != -7) if res[k].dtype.kind == "i" else not np.isnan(res[k]).any()
               for k in ("ll", "cutoff", "top", "n_tail", "tail", "sums", "psums"))


def check_raw(ll32, lens, got):
    """The fused tails `got` ({'cutoff', 'top', 'n_tail', 'tail', 'sums', 'flag'}) against `loglik_case.select_exact` and
    `loglik_case.sum_bounds` of the written matrix, and, for at most 512 rows, bit for bit against `l2hmc_loglik_tails` of it;
    returns the worst sum error over its bound."""
    from tests import loglik_case as lk
    S, n = ll32.shape
    eff = np.full(n, tail_len(S), dtype=np.int64) if lens is None else lens
    ex = lk.select_exact(ll32, eff)
    assert int(got["flag"][0]) == 0
    assert np.array_equal(bits(got["cutoff"]), bits(ex["cutoff"])) and np.array_equal(bits(got["top"]), bits(ex["top"]))
    assert np.array_equal(got["n_tail"], ex["n_tail"]) and np.all(got["n_tail"] <= eff)
    assert got["tail"].shape == (n, int(eff.max()))
    for i in range(n):
        L = int(ex["n_tail"][i])
        assert np.all(np.isposinf(got["tail"][i, L:])), i
        assert sorted(lk.keys(got["tail"][i, :L]).tolist()) == [p[0] for p in ex["pairs"][i]], i
    ref, bound = lk.sum_bounds(ll32, ex)
    err = np.abs(got["sums"] - ref)
    worst = float(np.max(err / bound))
    print("worst sum error / bound %.3g" % worst)
    assert np.all(err <= bound), worst
    if n <= 512:                                             # ... and they are the matrix gather's own sums: the same terms, the same order
        mat = lk.device_raw(ll32, lens, want_pos=False)
        assert np.array_equal(bits(got["sums"]), bits(mat["sums"]))
    return worst


def predictive_of(psums, consts_sat, S):
    """mean mu, lppd_i, mean ll and p_waic_i of the raw sums (4, m) of `l2hmc_glm_predict`, finished by `predictive.finish` as
    `glm.Glm.waic` finishes them."""
    from l2hmc_amd import predictive
    with np.errstate(all="ignore"):
        f = predictive.finish({"sum_p": psums[0], "sum_lik": psums[1], "sum_ll": psums[2], "sum_ll2": psums[3],
                               "log_sum_lik": np.log(psums[1]) + consts_sat, "n_draws": S})
    return {"mean_mu": psums[0] / S, "lppd_i": f.lppd_i, "mean_ll": psums[2] / S, "p_waic_i": f.p_waic_i}, f
