"""GPU: the three entries of csrc/glm.hip for the binomial and the negative-binomial family (csrc/glm_binomial.hip; a
log-likelihood of THREE row constants: `row_constants<NB, KC, true>` skips sat, the gather keeps a fifth row of `rowc`, the
predictive sums at NTM = 8 read sat and the third constant again for every element) called straight
(`binomial_case.device_raw`: outputs filled with NaN / -7 before the call and 8 guard elements longer than the entry is told),
where tests/test_gpu_binomial_glm.py does not reach -- the mirror of tests/test_gpu_glm_geometries.py:

  geometries    `binomial_case.GEOM_SHAPES`, (70, 35, d) with NT / NTM = 3 / 4 (d = 33, 40), 5 / 8 (65), 6 / 8 (96), 7 / 8 (100,
                112), binomial and negative binomial (phi = 10: its own predictive instantiation): every in-range element is
                written, no guard element is, the tails are the exact selection of the written matrix, the outputs are the
                public route's bit for bit, rows [17, n) alone give the bits they have inside the whole, and matrix and
                predictive numbers lie inside `binomial_case.ll_bounds`;
  long          `binomial_case.LONG`: S > 131072 with three rows, where the gather's segments are no multiple of a tile and
                its loads are late with three constants in flight (binomial and negative binomial phi = 0.5);
  edges         `binomial_case.edge_case`: a row whose e^-|t| is denormal or zero, the cancellation y t - m softplus(t) at
                y = m, 2^24 trials, a likelihood that underflows against sat in every draw, a constant row -- each sharing a
                16-row block with ordinary rows;
  dispersion    `binomial_case.nb_edge_case`: phi = 1e-3 and 1e4 with a count of 100000.
No figure here comes from the device: the bounds are `binomial_case.ll_bounds` and `loglik_case.sum_bounds`, the gates of the
finished numbers the K_* of tests/binomial_case.py, the rest is equality."""
import numpy as np
import pytest

from tests import binomial_case as bc
from tests import glm_case as gc
from tests import loglik_case as lk

pytestmark = pytest.mark.gpu
RAW = ("ll", "cutoff", "top", "n_tail", "sums")
FAMILIES = [("binomial", None), ("negbinomial", 10.0)]
_EDGE = {}


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _sorted_tail(tail):
    return np.sort(lk.keys(tail), axis=1)                    # (monotone keys: the +inf pads last; a tail never holds a NaN)


def _public(m, Wd, lens):
    """The public route's outputs under the names of `device_raw`; 'sum_mu' apart (the host has multiplied the negative
    binomial's by phi)."""
    t = {k: v.cpu().numpy() for k, v in m._glm.loo_tails(Wd, tail_len_row=lens).items()}
    s = m._glm.pointwise_sums(Wd)
    return {"ll": m.log_lik(Wd).cpu().numpy(), "cutoff": t["cutoff"], "top": t["top"], "n_tail": t["n_tail"], "tail": t["tail"],
            "sums": np.stack([t["body"], t["body_sq"], t["lik"]]), "flag": t["flag"],
            "psums": np.stack([s["sum_lik"], s["sum_ll"], s["sum_ll2"]]), "sum_mu": s["sum_mu"]}


def _same(a, b, cols=slice(None), what=""):
    """Two results of `device_raw` equal bit for bit (NaNs by position), `a` on the rows `cols`; the tails as sorted rows
    (their slot order is arrival order)."""
    for k in RAW + ("psums",):
        assert gc.same_bits(a[k][..., cols], b[k]), (what, k)
    _same_tails(a, b, cols, what)


def _same_tails(a, b, cols, what):
    assert np.array_equal(_sorted_tail(a["tail"][cols])[:, :b["tail"].shape[1]], _sorted_tail(b["tail"])), (what, "tail")
    past = np.sort(a["tail"][cols], axis=1)[:, b["tail"].shape[1]:]
    assert np.all(np.isposinf(past)), (what, "pads")
    assert int(a["flag"][0]) == int(b["flag"][0]) == 0


def _same_as_public(res, pub, scale, what):
    """`device_raw`'s result against `_public`: psums[1:] bit for bit, and sum_mu times the family's `mean_scale` (one float64
    product on the host, restated)."""
    for k in RAW:
        assert gc.same_bits(res[k], pub[k]), (what, k)
    assert gc.same_bits(res["psums"][1:], pub["psums"]), (what, "psums[1:]")
    assert gc.same_bits(res["psums"][0] if scale == 1.0 else res["psums"][0] * scale, pub["sum_mu"]), (what, "sum_mu")
    _same_tails(res, pub, slice(None), what)


def _predictive(c, res, S):
    """mean, lppd_i, mean ll and p_waic_i of the raw predictive sums, finished as `Glm.waic` finishes them, and the Summary."""
    sat = bc.model(c)._glm.consts[2].astype(np.float64)
    got, f = gc.predictive_of(res["psums"], sat, S)
    if c["kind"] == "negbinomial":
        got["mean_mu"] = got["mean_mu"] * c["phi"]
    return got, f


def _shares(c, res, S):
    """The share of each bound of `binomial_case.ll_bounds` the matrix and the predictive numbers use."""
    ll64, _ = bc.log_lik(c)
    b, ref = bc.ll_bounds(c), bc.restatement(c)
    got, f = _predictive(c, res, S)
    shares = {"ll": float(np.max(np.abs(res["ll"].astype(np.float64) - ll64) / b["B"]))}
    shares.update({k: float(np.max(np.abs(got[k] - ref[k]) / b[k])) for k in got})
    return shares, f


# ---- every geometry, with poisoned outputs and guards --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,phi", FAMILIES)
@pytest.mark.parametrize("S,n,d", bc.GEOM_SHAPES)
def test_raw_entries_write_every_element_and_no_other(S, n, d, kind, phi):
    """With one tail length and with per-row lengths that include 0, 1, 4, 5 and S // 5: no in-range element keeps its fill,
    every guard element does, `check_raw` holds (the exact selection of the written matrix, `l2hmc_loglik_tails` of it bit for
    bit), the outputs are the public route's bit for bit, rows [17, n) in a call of their own give the bits they have inside
    the whole; the matrix within B_si and mean, lppd_i, mean ll and p_waic_i inside `ll_bounds`; at d = 100, binomial,
    `predict_mean` of the model's own rows handed back as new ones returns the bits of sum_mu / S."""
    c = bc.case(S, n, d, kind, phi)
    m, Wd = bc.model(c), _dev(c["W"])
    scale = 1.0 if kind == "binomial" else phi
    for lens in (None, lk.lengths_for(S, n)):
        res = bc.device_raw(c, Wd, lens)
        assert gc.all_written(res), [k for k in RAW + ("psums", "tail") if res[k].dtype.kind == "f" and np.isnan(res[k]).any()]
        assert gc.guards_untouched(res), res["guards"]
        gc.check_raw(res["ll"], lens, res)
        _same_as_public(res, _public(m, Wd, lens), scale, "public route")
        part = bc.device_raw(c, Wd, lens, rows=(17, n))
        assert gc.all_written(part) and gc.guards_untouched(part)
        _same(res, part, cols=slice(17, n), what="rows [17, n)")
    shares, f = _shares(c, res, S)
    print(kind, phi, (S, n, d), "NT / NTM %d / %d " % (-(-d // 16), 4 if d <= 64 else 8), " ".join("%s %.3g" % kv for kv in shares.items()))
    assert all(v <= 1.0 for v in shares.values()), shares
    assert f.n_underflow == 0 and f.n_draws == S
    if kind == "binomial" and d == 100:
        new = m.predict_mean(Wd, X=c["X"], offset=c["offset"], trials=c["trials"])
        assert gc.same_bits(new, res["psums"][0] / S)


# ---- long histories where the loads are late -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,phi", [("binomial", None), ("negbinomial", 0.5)])
@pytest.mark.parametrize("S,n,d", bc.LONG)
def test_ragged_segment_tiles_under_late_loads(S, n, d, kind, phi):
    """`glm_case.check_raw` (the exact selection of the written matrix, its sums inside `loglik_case.sum_bounds`, bit equality
    with `l2hmc_loglik_tails` of it) with one tail length and with per-row lengths; the matrix within B_si of the float64
    likelihood; the mean, lppd_i, mean ll and p_waic_i within `binomial_case.ll_bounds`.  (The three binomial rows are y = 0 of
    50, 1 of 1 and 50 of 50, whose third constant and sat are both 0: the negative-binomial cases are the ones that tell the
    gather's fifth row of constants and the streamed sat from zeros.)"""
    c = bc.case(S, n, d, kind, phi)
    Wd = _dev(c["W"])
    for lens in (None, lk.lengths_for(S, n)):
        res = bc.device_raw(c, Wd, lens)
        assert gc.all_written(res) and gc.guards_untouched(res)
        gc.check_raw(res["ll"], lens, res)
    shares, f = _shares(c, res, S)
    print(kind, phi, (S, n, d), " ".join("%s %.3g" % kv for kv in shares.items()))
    assert all(v <= 1.0 for v in shares.values()), shares
    assert f.n_underflow == 0 and f.n_draws == S


# ---- the edges of the likelihood ---------------------------------------------------------------------------------------------
def _edge(S):
    """The edge case, `ordinary`, its model, the draws on the device and the raw outputs with one tail length: computed once."""
    if S not in _EDGE:
        c, ordinary = bc.edge_case(S)
        Wd = _dev(c["W"])
        _EDGE[S] = (c, ordinary, bc.model(c), Wd, bc.device_raw(c, Wd))
    return _EDGE[S]


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_matrix_against_float64(S):
    """Every element finite (the family's promise: nothing overflows) and within B_si, which is absolute (it carries 8 u m) and
    so speaks of the `certain` row's flush to zero too; the `certain` row below the float32 normal range in every draw; the
    `constant` row one bit pattern.  (The `saturated` row is not held to `log_lik32`: the device's fma(-y, t, m sp) keeps the
    rounding residue of m sp where numpy's two products cancel to 0.  B covers both.)"""
    c, _, _, _, res = _edge(S)
    at = bc.EDGE_ROWS
    assert gc.all_written(res) and gc.guards_untouched(res) and int(res["flag"][0]) == 0
    ll32 = res["ll"]
    ll64, _ = bc.log_lik(c)
    share = np.abs(ll32.astype(np.float64) - ll64) / bc.ll_bounds(c)["B"]
    print("S = %d: worst |ll32 - ll64| / bound %.3g; by edge row %s" % (S, share.max(), " ".join("%s %.3g" % (k, share[:, i].max()) for k, i in at.items())))
    assert np.all(np.isfinite(ll32)) and share.max() <= 1.0
    assert np.all(np.abs(ll32[:, at["certain"]]) < 2.0 ** -126)
    assert np.all(gc.bits(ll32[:, at["constant"]]) == gc.bits(ll32[:1, at["constant"]])[0])


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_tails_are_the_exact_selection_of_the_matrix(S):
    """With one tail length and with per-row lengths `check_raw` holds: cutoff, top, n_tail and the sorted tail are
    `loglik_case.select_exact` of the written matrix, the sums lie inside `sum_bounds` and equal `l2hmc_loglik_tails` of the
    written matrix bit for bit.  The `constant` row has cutoff == top, an empty tail, body and body_sq equal to S exactly
    (S terms e^0) and its third sum inside `sum_bounds`."""
    c, _, _, Wd, first = _edge(S)
    ll32, n = first["ll"], bc.EDGE_N
    for lens in (None, lk.lengths_for(S, n)):
        res = first if lens is None else bc.device_raw(c, Wd, lens)
        assert gc.guards_untouched(res) and gc.same_bits(res["ll"], ll32)
        worst = gc.check_raw(ll32, lens, res)
        print("S = %d, %s: worst tail sum error / bound %.3g" % (S, "one length" if lens is None else "per-row lengths", worst))
    res, k = first, bc.EDGE_ROWS["constant"]
    assert gc.bits(res["cutoff"])[k] == gc.bits(res["top"])[k] == gc.bits(ll32[:1, k])[0] and res["n_tail"][k] == 0
    assert res["sums"][0, k] == S and res["sums"][1, k] == S
    ref, bound = lk.sum_bounds(ll32, lk.select_exact(ll32, np.full(n, gc.tail_len(S), dtype=np.int64)))
    assert abs(res["sums"][2, k] - ref[2, k]) <= bound[2, k] and ref[2, k] == S
    assert np.all(np.isfinite(res["sums"])) and np.all(res["n_tail"] <= gc.tail_len(S))


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_finished_numbers_are_those_of_the_materialised_route(S):
    """`loo` against `loo_from_log_lik(select="fused")` of the written matrix, with and without r_eff: the same NaN / inf
    pattern and the same bits elsewhere (the raw material is the same bit for bit and the finish is the same code); every
    ordinary row finite, and on those rows the float64 host route within the K_* delta_i gates of tests/binomial_case.py
    (every edge row is an infinite-khat row on the host by construction: tests/test_binomial_cpu.py)."""
    from l2hmc_amd import psis
    c, ordinary, m, Wd, first = _edge(S)
    n = bc.EDGE_N
    dev = _dev(first["ll"])
    delta = bc.ll_bounds(c)["delta"][ordinary]
    for r in (None, lk.r_eff_for(n)):
        got, ref = m.loo(Wd, r_eff=r), psis.loo_from_log_lik(dev, r_eff=r, select="fused")
        for k in ("khat", "elpd_loo_i", "lppd_i", "n_tail") + (("n_eff", "mcse_elpd_loo_i", "tail_len_row") if r is not None else ()):
            assert gc.same_bits(np.asarray(got[k]), np.asarray(ref[k])), (k, got[k], ref[k])
        assert np.all(np.isfinite(got.elpd_loo_i[ordinary])) and np.all(np.isfinite(got.khat[ordinary]))
        host = m.loo(c["W"], r_eff=r)
        assert np.all(np.isfinite(host.khat[ordinary]))
        shares = {"khat": np.max(np.abs(got.khat[ordinary] - host.khat[ordinary]) / (bc.K_KHAT * delta)),
                  "elpd_loo_i": np.max(np.abs(got.elpd_loo_i[ordinary] - host.elpd_loo_i[ordinary]) / (bc.K_ELPD * delta))}
        if r is not None:
            assert np.all(np.isfinite(got.n_eff[ordinary])) and np.all(np.isfinite(got.mcse_elpd_loo_i[ordinary]))
            shares["n_eff"] = np.max(gc.rel(got.n_eff[ordinary], host.n_eff[ordinary]) / (bc.K_NEFF * delta))
            shares["mcse"] = np.max(gc.rel(got.mcse_elpd_loo_i[ordinary], host.mcse_elpd_loo_i[ordinary]) / (bc.K_MCSE * delta))
        print("S = %d, r_eff %s: ordinary rows use %s of the gates" % (S, "given" if r is not None else "none",
                                                                      " ".join("%s %.3g" % (k, float(v)) for k, v in shares.items())))
        assert all(float(v) <= 1.0 for v in shares.values()), shares


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_ordinary_rows_do_not_depend_on_the_edge_rows(S):
    """The 32 ordinary rows equal, bit for bit, the same rows of the model without the edge rows: matrix, cutoff, top, n_tail,
    the sorted tail, the tail sums and the predictive sums, with one tail length and with per-row lengths."""
    c, ordinary, _, Wd, first = _edge(S)
    lens = lk.lengths_for(S, bc.EDGE_N)
    assert lens[ordinary].max() == lens.max()
    plain = bc.select_rows(c, ordinary)
    for ln, res in ((None, first), (lens, bc.device_raw(c, Wd, lens))):
        alone = bc.device_raw(plain, Wd, None if ln is None else ln[ordinary])
        assert gc.all_written(alone) and gc.guards_untouched(alone)
        _same(res, alone, cols=ordinary, what="without the edge rows")


@pytest.mark.parametrize("S", gc.EDGE_S)
def test_edge_predictive_sums_follow_the_written_matrix(S):
    """sum ll, sum ll^2 and sum exp(ll - sat) against extended-precision sums of the written float32 matrix: S 2^-53 relative to
    the sum of the terms' magnitudes for the additions in whatever order (sum ll^2 is one fma per term), and per term of the
    third the bound of `loglik_case.sum_bounds` -- (|ll - sat| + 2) (2^-52 + the reference's epsilon).  `underflow` and
    `many_trials` have sum_lik = 0 and lppd_i = -inf and are the two rows `n_underflow` counts, as on the host route.  The
    mean, sum_mu / S, within mean Bmean on every row: at 2^24 trials the one check that the weight reaches `mean` unrounded."""
    c, _, m, Wd, res = _edge(S)
    at, ld = bc.EDGE_ROWS, np.longdouble
    ps, ll = res["psums"], res["ll"].astype(ld)
    s = m._glm.pointwise_sums(Wd)
    assert gc.same_bits(ps, np.stack([s["sum_mu"], s["sum_lik"], s["sum_ll"], s["sum_ll2"]]))
    sat = m._glm.consts[2].astype(ld)
    u = ld(2.0) ** -53
    with np.errstate(all="ignore"):
        lik = np.exp(ll - sat)
        per_term = np.where(lik == 0, ld(0), lik * (np.abs(ll - sat) + 2) * (2 * u + ld(np.finfo(ld).eps)))      # (a zero term is exact)
        want = {1: (lik.sum(axis=0), per_term.sum(axis=0) + S * u * lik.sum(axis=0)),
                2: (ll.sum(axis=0), S * u * np.abs(ll).sum(axis=0)), 3: ((ll * ll).sum(axis=0), S * u * (ll * ll).sum(axis=0))}
        for k, (ref, bound) in want.items():
            ref, bound = ref.astype(np.float64), bound.astype(np.float64)
            assert np.all(np.isfinite(ref)) and np.all(np.isfinite(ps[k]))
            share = np.where(ps[k] == ref, 0.0, np.abs(ps[k] - ref) / bound)
            print("S = %d: %s uses %.3g of its bound" % (S, ("", "sum_lik", "sum_ll", "sum_ll2")[k], share.max()))
            assert np.all(np.abs(ps[k] - ref) <= bound), (k, ps[k], ref, bound)
    dead = [at["underflow"], at["many_trials"]]
    f, host = m.waic(Wd), m.waic(c["W"])
    assert np.all(ps[1][dead] == 0.0) and np.all(np.isneginf(f.lppd_i[dead])) and np.count_nonzero(ps[1] == 0.0) == 2
    assert f.n_underflow == host.n_underflow == 2
    b, ref = bc.ll_bounds(c), bc.restatement(c)
    share = np.abs(ps[0] / S - ref["mean_mu"]) / b["mean_mu"]
    print("S = %d: mean / bound %.3g (at 2^24 trials %.3g)" % (S, share.max(), share[at["many_trials"]]))
    assert np.all(share <= 1.0), share


# ---- the dispersion far from 0.5 and 10 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("phi", bc.NB_EDGE_PHIS)
def test_dispersion_edges(phi):
    """`binomial_case.nb_edge_case`: the matrix within B_si, `check_raw` with both kinds of tail length, the finished numbers
    the materialised route's bits, and the predictive numbers inside `ll_bounds` -- lppd_i on the rows where the float64 host
    route's is finite: the count of 100000 at phi = 1e4 underflows against sat in every draw, lppd_i = -inf on either route,
    and it is the one row `n_underflow` counts."""
    from l2hmc_amd import psis
    c = bc.nb_edge_case(phi)
    S, n = c["W"].shape[0], c["X"].shape[0]
    m, Wd = bc.model(c), _dev(c["W"])
    for lens in (None, lk.lengths_for(S, n)):
        res = bc.device_raw(c, Wd, lens)
        assert gc.all_written(res) and gc.guards_untouched(res)
        gc.check_raw(res["ll"], lens, res)
    dev = _dev(res["ll"])
    for r in (None, lk.r_eff_for(n)):
        got, ref = m.loo(Wd, r_eff=r), psis.loo_from_log_lik(dev, r_eff=r, select="fused")
        for k in ("khat", "elpd_loo_i", "lppd_i", "n_tail") + (("n_eff", "mcse_elpd_loo_i", "tail_len_row") if r is not None else ()):
            assert gc.same_bits(np.asarray(got[k]), np.asarray(ref[k])), (k, got[k], ref[k])
    ll64, _ = bc.log_lik(c)
    b, want = bc.ll_bounds(c), bc.restatement(c)
    got, f = _predictive(c, res, S)
    host = m.waic(c["W"])
    live = np.isfinite(host.lppd_i)
    assert f.n_underflow == host.n_underflow == int((~live).sum()) and np.array_equal(np.isfinite(got["lppd_i"]), live)
    shares = {"ll": float(np.max(np.abs(res["ll"].astype(np.float64) - ll64) / b["B"]))}
    for k in got:
        rows = live if k == "lppd_i" else slice(None)
        shares[k] = float(np.max((np.abs(got[k] - want[k]) / b[k])[rows]))
    print("phi = %g:" % phi, " ".join("%s %.3g" % kv for kv in shares.items()), "rows underflowed: %d" % f.n_underflow)
    assert all(v <= 1.0 for v in shares.values()), shares
