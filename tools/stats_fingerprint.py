#!/usr/bin/env python
"""Bit-for-bit fingerprint of the host side of the history statistics (`diagnostics`, `quantiles`, `multivariate`, `predictive`,
`func_utils.acl_spectrum` and their `sharding` forms): one SHA-256 per host code path, over the raw bytes of every array a call
returns, each case at the smallest shape that still takes its path.  Public API only, so the same file runs against two
versions of `l2hmc_amd/*.py` on ONE build of the library (`L2HMC_LIB=`): a host-side refactor must leave every line as it was.

    python tools/stats_fingerprint.py                       # numpy, a CPU tensor and, with a GPU, four forms of a device tensor
    python tools/stats_fingerprint.py --cpu                 # the host inputs only
    python tools/stats_fingerprint.py --kernels             # the device kernels that share csrc/draw_tiles.hpp and radix_select.hpp
    python tools/stats_fingerprint.py --ranks 2 --backend gloo|nccl --input numpy|device      # chains sharded 2 | 4
    python tools/stats_fingerprint.py --time                # median host time of `describe` and `loo(r_eff=)` on the tiny device history

The history is a seeded AR(1) of 40 steps, 6 chains and 3 coordinates whose means and scales differ per coordinate.  `--kernels`
runs ONE version of the Python against two builds of the library instead: `pointwise_sums`, `loo_tails` (with and without a
tail length per row), `order_statistics`, `relative_eff` and the statistics of a `glm.Glm` over Poisson counts (`log_lik`,
`pointwise_sums`, `loo_tails`, `relative_eff`) are declared bitwise reproducible, so a refactor of their kernels must leave
every line as it was too."""
import argparse
import hashlib
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import diagnostics, func_utils, glm, multivariate, predictive, psis, quantiles, sharding

STEPS, CHAINS, DIM, ROWS, SCALE = 40, 6, 3, 5, 1.7
SPLIT = 2                                 # --ranks 2: rank 0 holds chains [0, 2), rank 1 chains [2, 6)
RANKS33 = np.arange(33) * 7               # 33 ranks: two chunks of at most 32
PROBS = (0.1, 0.5, 0.9)
R_EFF = np.array([0.3, 0.5, 1.0, np.nan, 2.0])   # per-row tail lengths 48, 48, 47, 47, 33 of the 240 draws; one NaN
# (S, n, d) of tests/loo_case.case, the smallest shapes that reach every branch of the shared tile loop: 1, 2, 4, 8 compiled
# feature tiles; two row groups of the predict plan at four blocks per wave; five tiles per chunk with a last tile of 9 draws, a
# last chunk of one tile and dead waves; no tail at all (M = 0)
KERNEL_SHAPES = ((70, 35, 5), (523, 33, 17), (70, 35, 40), (300, 50, 128), (4099, 100, 25), (65609, 33, 1), (4, 3, 2))
# the Poisson kernels alone: n_draws > 131072 cuts the gather's segments off a tile boundary (tests/test_gpu_glm.py: 69-draw
# segments at d = 2; tests/test_gpu_glm_geometries.py: 65-draw segments and a short last one under the late loads of d = 40)
GLM_LONG_SHAPES = ((140001, 3, 2), (131073, 3, 40))


def history():
    rng = np.random.RandomState(17)
    X = np.empty((STEPS, CHAINS, DIM))
    X[0] = rng.randn(CHAINS, DIM)
    for t in range(1, STEPS):
        X[t] = 0.7 * X[t - 1] + rng.randn(CHAINS, DIM)
    return X * np.array([0.5, 1.0, 3.0]) + np.array([-2.0, 0.25, 10.0])


def rows():
    rng = np.random.RandomState(18)
    return 0.2 * rng.randn(ROWS, DIM), (rng.rand(ROWS) < 0.5).astype(np.float64)


def sha(result):
    h = hashlib.sha256()

    def feed(v):
        if isinstance(v, dict):
            for k in sorted(v):
                h.update(k.encode())
                feed(v[k])
        elif isinstance(v, (tuple, list)):
            for e in v:
                feed(e)
        elif v is not None:
            h.update(np.ascontiguousarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v).tobytes())
    feed(result)
    return h.hexdigest()


def cases(X):
    """(name, call) of every single-process statistic on the history X (numpy or a tensor, anywhere)."""
    rx, ry = rows()
    thresholds = np.array([-2.0, 0.25, 10.0])
    for split in (True, False):
        for lag in (3, None):
            yield "summarize split=%d max_lag=%s" % (split, lag), lambda s=split, g=lag: diagnostics.summarize(X, max_lag=g, split=s)
    yield "chain_sums_below", lambda: diagnostics.chain_sums_below(X, thresholds)
    yield "order_statistics 33 ranks", lambda: quantiles.order_statistics(X, RANKS33)
    yield "quantiles", lambda: quantiles.quantiles(X, PROBS)
    yield "describe", lambda: quantiles.describe(X)
    yield "covariance (240, 3)", lambda: multivariate.covariance(X.reshape(STEPS * CHAINS, DIM))
    yield "multi_ess", lambda: multivariate.multi_ess(X)
    yield "waic", lambda: predictive.waic(X, rx, ry)
    yield "predict_proba", lambda: predictive.predict_proba(X, rx)
    yield "log_predictive_density", lambda: predictive.log_predictive_density(X, rx, ry)
    yield "loo", lambda: predictive.loo(X, rx, ry)
    yield "acl_spectrum", lambda: func_utils.acl_spectrum(X, SCALE)
    yield from loo_cases(X, rx, ry)


def loo_cases(X, rx, ry):
    """Every host route of `relative_eff`, `loo(r_eff=)`, `loo_tails`, `loo_finish` and the `psis` module on the same history;
    the kernel finish and the row groups only where the history lies on a device."""
    on_device = torch.is_tensor(X) and X.is_cuda
    like = (lambda a: torch.as_tensor(a).to(X.device)) if torch.is_tensor(X) else (lambda a: a)
    for split in (False, True):
        for lag in (5, None):
            yield ("relative_eff split=%d max_lag=%s" % (split, lag),
                   lambda s=split, g=lag: predictive.relative_eff(X, rx, ry, max_lag=g, split=s))
    lens = predictive.tail_len_rows(R_EFF, STEPS * CHAINS)
    assert lens.tolist() == [48, 48, 47, 47, 33]

    def tails(per_row):
        t = predictive.loo_tails(X, rx, ry, tail_len_row=lens if per_row else None)
        if torch.is_tensor(t["tail"]):
            t["tail"] = torch.sort(t["tail"], dim=-1).values                        # its slot order is arrival order
        return t

    finishes = ("torch", "kernel") if on_device else ("torch",)
    yield "loo r_eff=auto", lambda: predictive.loo(X, rx, ry, r_eff="auto")
    yield "loo_tails", lambda: tails(False)
    yield "loo_tails tail_len_row", lambda: tails(True)
    for f in finishes:
        yield "loo r_eff=array finish=%s" % f, lambda f=f: predictive.loo(X, rx, ry, r_eff=R_EFF, finish=f)
        yield "loo_finish finish=%s" % f, lambda f=f: predictive.loo_finish(tails(False), finish=f)
        yield "loo_finish r_eff finish=%s" % f, lambda f=f: predictive.loo_finish(tails(True), finish=f, r_eff=R_EFF)
    if on_device:
        small = 4 * 48 * 2                                    # two rows per group: three groups
        yield "loo finish=kernel", lambda: predictive.loo(X, rx, ry, finish="kernel")
        for f in finishes:
            yield "loo 3 groups finish=%s" % f, lambda f=f: predictive.loo(X, rx, ry, max_tail_bytes=small, finish=f)
            yield ("loo r_eff=array 3 groups finish=%s" % f,
                   lambda f=f: predictive.loo(X, rx, ry, max_tail_bytes=small, finish=f, r_eff=R_EFF))
    W = (X.detach().cpu().numpy() if torch.is_tensor(X) else X).astype(np.float64).reshape(STEPS * CHAINS, DIM)
    ll = -np.logaddexp(0.0, -(W @ rx.T) * (2.0 * ry - 1.0))   # the (240, 5) pointwise log-likelihood matrix
    M = predictive.loo_tail_len(STEPS * CHAINS)
    top = -np.sort(ll, axis=0)[:M + 1]                        # the M + 1 largest ratios -ll of every column, descending
    lam, cutoff = np.ascontiguousarray(top[:M].T), top[M].copy()
    n_tail = (top[:M] > cutoff[None, :]).sum(axis=0).astype(np.int64)
    yield "psis.psis", lambda: psis.psis(like(-ll))
    yield "psis.psis 1-d", lambda: psis.psis(like(-ll[:, 0].copy()))
    yield "psis.psis weights=False", lambda: psis.psis(like(-ll), weights=False)
    yield "psis.loo_from_log_lik float32", lambda: psis.loo_from_log_lik(like(ll.astype(np.float32)))
    yield "psis.loo_from_log_lik float64", lambda: psis.loo_from_log_lik(like(ll))
    for w in (False, True):
        yield "psis.smooth_tails weights=%d" % w, lambda w=w: psis.smooth_tails(like(lam), like(n_tail), like(cutoff), weights=w)


def _sorted_tail(tails):
    tails["tail"] = torch.sort(tails["tail"], dim=-1).values                        # its slot order is arrival order
    return tails


def kernels():
    """One line per (statistic, shape) of the draw-tile and radix-select kernels: the logistic `pointwise_sums`, `loo_tails`
    (one tail length, then one per row), `order_statistics` and `relative_eff`, and the same of a Poisson `glm.Glm`."""
    from tests import glm_case, lik_stats_case, loglik_case, loo_case
    torch.cuda.set_device(0)
    cuda = lambda a: torch.as_tensor(a).cuda()  # noqa: E731
    line = lambda res, name, label: print("%s  %s %s" % (sha(res), name, label), flush=True)  # noqa: E731
    inputs = []
    for S, n, d in KERNEL_SHAPES:
        inputs.append(("(%d, %d, %d)" % (S, n, d),) + tuple(cuda(a) for a in loo_case.case(S, n, d)))
    W, X, y = (cuda(a) for a in loo_case.case(40 * 13, 33, 17))
    hist = W.reshape(40, 13, 17)[3:]                          # a base that is not 16-byte aligned
    assert hist.is_contiguous() and hist.data_ptr() % 16
    inputs.append(("(40, 13, 17)[3:], 33 rows", hist, X, y))
    for label, W, X, y in inputs:
        S = W.numel() // W.shape[-1]
        ranks = np.unique([0, 1, S // 3, S // 2, S - 2, S - 1])
        lens = loglik_case.lengths_for(S, X.shape[0])
        line(predictive.pointwise_sums(W, X, y), "pointwise_sums", label)
        line(_sorted_tail(predictive.loo_tails(W, X, y)), "loo_tails", label)
        line(_sorted_tail(predictive.loo_tails(W, X, y, tail_len_row=lens)), "loo_tails tail_len_row", label)
        line(quantiles.order_statistics(W, ranks), "order_statistics", label)
    for S, n, d in KERNEL_SHAPES + GLM_LONG_SHAPES:
        W, X, y, o = glm_case.case(S, n, d)
        label, Wd, model = "(%d, %d, %d)" % (S, n, d), cuda(W), glm.Glm(X, y, o)
        line(model.log_lik(Wd), "glm log_lik", label)
        line(model.pointwise_sums(Wd), "glm pointwise_sums", label)
        line(_sorted_tail(model.loo_tails(Wd)), "glm loo_tails", label)
        line(_sorted_tail(model.loo_tails(Wd, tail_len_row=loglik_case.lengths_for(S, n))), "glm loo_tails tail_len_row", label)
    # the history forms: the smallest (steps, chains, d, rows) of tests/lik_stats_case.py, whole chains and split ones
    M, N, d, rho, max_lag, _ = min(lik_stats_case.FIXTURES, key=lambda f: f[0] * f[1] * f[2])
    W, X, y = lik_stats_case.ar1_case(M, N, d, rho)
    rng = np.random.RandomState(19)
    o = rng.uniform(-1.0, 2.0, size=X.shape[0]).astype(np.float32)
    counts = rng.poisson(np.exp(X.astype(np.float64) @ W.reshape(-1, d).mean(axis=0) + o)).astype(np.float32)
    Wd, model = cuda(W), glm.Glm(X, counts, o)
    for split in (False, True):
        label = "(%d, %d, %d), %d rows, split=%d" % (M, N, d, X.shape[0], split)
        lag = min(max_lag, (M // 2 if split else M) - 1)
        line(predictive.relative_eff(Wd, X, y, max_lag=lag, split=split), "relative_eff", label)
        line(model.relative_eff(Wd, max_lag=lag, split=split), "glm relative_eff", label)


def device_inputs(X, dev):
    """The history on the device, four ways: the first reads in place, so does the second, the last two are copied."""
    x32 = torch.as_tensor(X.astype(np.float32)).to(dev)
    longer = torch.zeros((STEPS + 10, CHAINS, DIM), dtype=torch.float32, device=dev)
    longer[10:] = x32
    wider = torch.zeros((STEPS, 2 * CHAINS, DIM), dtype=torch.float32, device=dev)
    wider[:, ::2] = x32
    assert longer[10:].is_contiguous() and not wider[:, ::2].is_contiguous()
    return (("device float32", x32), ("device first-axis slice", longer[10:]), ("device float64", torch.as_tensor(X).to(dev)),
            ("device X[:, ::2]", wider[:, ::2]))


def single(cpu_only):
    X = history()
    inputs = [("numpy", X.astype(np.float32)), ("cpu tensor", torch.as_tensor(X.astype(np.float32)))]
    if not cpu_only:
        torch.cuda.set_device(0)
        inputs += device_inputs(X, torch.device("cuda", 0))
    for label, Xi in inputs:
        for name, call in cases(Xi):
            print("%s  %s: %s" % (sha(call()), label, name), flush=True)


def _rank(rank, world, port, backend, on_device, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    X = history().astype(np.float32)
    X = X[:, :SPLIT] if rank == 0 else X[:, SPLIT:]
    if on_device:
        dev = torch.device("cuda", rank % torch.cuda.device_count() if backend == "gloo" else rank)
        torch.cuda.set_device(dev)
        X = torch.as_tensor(X).to(dev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        rx, ry = rows()
        res = [("sharding.diagnostics", sharding.diagnostics(X)),
               ("sharding.describe", sharding.describe(X)),
               ("sharding.predictive", sharding.predictive(X, rx, ry)),
               ("sharding.multivariate", sharding.multivariate(X)),
               ("sharding.acl_spectrum", sharding.acl_spectrum(X, SCALE, CHAINS)),
               ("sharding.ess", np.float64(sharding.ess(X, SCALE, CHAINS)))]
        out.put((rank, [(name, sha(r)) for name, r in res]))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def sharded(world, backend, on_device):
    import torch.multiprocessing as mp
    if world != 2:
        raise SystemExit("the sharded fingerprint is defined for --ranks 2 (chains %d | %d)" % (SPLIT, CHAINS - SPLIT))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    out = ctx.SimpleQueue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, backend, on_device, out)) for r in range(world)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(150)
    if any(pr.exitcode != 0 for pr in procs):
        for pr in procs:
            if pr.is_alive():
                pr.kill()
        raise SystemExit("a rank failed or did not finish: exit codes %s" % [pr.exitcode for pr in procs])
    label = "%s, %s" % (backend, "device" if on_device else "numpy")
    for rank, lines in sorted(out.get() for _ in range(world)):
        for name, digest in lines:
            print("%s  %s, rank %d: %s" % (digest, label, rank, name), flush=True)


def timed():
    """The host side of a call is all there is to time on a history this small: median of 200 synchronised `describe`, then of
    200 synchronised `loo(r_eff=array)`."""
    torch.cuda.set_device(0)
    X = torch.as_tensor(history().astype(np.float32)).cuda()
    rx, ry = rows()
    for name, call in (("describe", lambda: quantiles.describe(X)), ("loo r_eff=array", lambda: predictive.loo(X, rx, ry, r_eff=R_EFF))):
        t = []
        for i in range(220):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        print("%s (40, 6, 3) on the device: median %.1f us over 200 calls after 20" % (name, 1e6 * float(np.median(t[20:]))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cpu", action="store_true", help="numpy and CPU-tensor inputs only (no GPU needed)")
    ap.add_argument("--kernels", action="store_true", help="the device kernels of predictive, quantiles and glm, shape by shape")
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--backend", default="gloo", choices=("gloo", "nccl"))
    ap.add_argument("--input", default="numpy", choices=("numpy", "device"))
    ap.add_argument("--time", action="store_true")
    a = ap.parse_args()
    if a.time:
        timed()
    elif a.kernels:
        kernels()
    elif a.ranks > 1:
        sharded(a.ranks, a.backend, a.input == "device")
    else:
        single(a.cpu)


if __name__ == "__main__":
    main()
