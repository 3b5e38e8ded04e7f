#!/usr/bin/env python
"""Bit-for-bit fingerprint of the host side of training and sampling (GPU box): one SHA-256 per code path of the Python that
marshals a launch, each case at the smallest shape that still takes its path.  Public API only, so the same file runs against
two versions of `l2hmc_amd/*.py` on ONE build of the library (`L2HMC_LIB=`): a host-side refactor must leave every line as it
was.

    python tools/train_fingerprint.py [--engine | --host-time]

`--engine`: the cases of the GEMM engine's host path alone (ENGINE_CASES below), for two builds of the library under one Python.

Training cases: the hash covers the bytes of `theta`, `m`, `v`, the returned chain state and the float64 loss after three seeded
`step` (`sampler_step`) calls.  Sampling cases: the bytes of `x_hist` and `p` of one `Dynamics.run` of three proposals."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from l2hmc_amd import Dynamics, LogisticRegression, LogisticTrainer, distributions as D, layers, vae
from l2hmc_amd.training import SplitTrainer, Trainer

N_CHAINS, STEPS = 64, 3


class Opaque(object):
    """the same function and variables as `net`, with nothing for the Dynamics to recognise: caller-supplied nets"""

    def __init__(self, net):
        self._net = net

    def __call__(self, inp):
        return self._net(inp)

    def parameters(self):
        return self._net.parameters()


def seeded():
    np.random.seed(7)                    # the masks (numpy's global stream, like the reference)
    torch.manual_seed(7)                 # the initial weights


def dynamics(d, energy, H=10, T=10, opaque=False, **kw):
    seeded()
    factory = layers.stq_network(H)
    if opaque:
        def factory(x_dim, scope, factor, make=factory):
            return Opaque(make(x_dim, scope=scope, factor=factor))
    return Dynamics(d, energy, T=T, eps=0.1, net_factory=factory, **kw)


def icg(d):
    return D.Gaussian(np.zeros(d), np.diag(np.logspace(-2, 2, d))).get_energy_function()


def dense(d):
    R = np.linalg.qr(np.random.RandomState(1).randn(d, d))[0]
    return D.Gaussian(np.zeros(d), (R * np.logspace(-1, 1, d)) @ R.T).get_energy_function()


def scg2d():
    return D.Gaussian(np.zeros(2), np.array([[50.05, -49.95], [-49.95, 50.05]])).get_energy_function()


def mog2d():
    return D.GMM([np.array([2.0, 0.0]), np.array([-2.0, 0.0])], [0.1 * np.eye(2), 0.1 * np.eye(2)], [0.5, 0.5]).get_energy_function()


def logistic(n=32, d=8):
    rng = np.random.RandomState(2)
    X = rng.randn(n, d)
    y = (rng.rand(n) < 1.0 / (1.0 + np.exp(-X @ rng.randn(d)))).astype(np.float64)
    return LogisticRegression(X, y, prior_var=4.0).get_energy_function()


def quadratic(x):                        # a callable energy: U and grad U by callback, Hessian-vector products by double backward
    return 0.5 * (x * x * x.new_tensor([1.0, 4.0, 0.25])).sum(1) + 0.1 * torch.cos(x).sum(1)


def tempered(dyn):
    dyn.use_temperature, dyn.temperature = True, 2.5
    return dyn


def stepped(dyn):
    dyn.eps_override = 0.05
    return dyn


def sha(*parts):
    h = hashlib.sha256()
    for t in parts:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).tobytes())
    return h.hexdigest()


def start(d, n=N_CHAINS):
    return torch.as_tensor(np.random.RandomState(3).randn(n, d).astype(np.float32)).cuda()


def train(dyn, cls, expect):
    tr = cls(dyn, seed=11)
    assert type(tr) is expect, (type(tr), expect)
    x = start(dyn.x_dim)
    for _ in range(STEPS):
        loss, _, x, _ = tr.step(x)
    return sha(tr.theta, tr.m, tr.v, x, np.float64(float(loss)))


def image_sampler(n_pix=16, d=4, H=8, enc_hidden=8, dec_hidden=8, n=32, T=5, hmc=False):
    """the image-conditioned sampler of the VAE experiment (default: 16 pixels, latent 4, hidden 8, 32 chains) and its images"""
    seeded()
    enc = vae.make_encoder_sampler(n_pix, enc_hidden, H)
    dyn = Dynamics(d, vae.VAEPosterior(vae.make_decoder(d, dec_hidden, n_pix)).get_energy_function(), T=T, eps=0.1,
                   net_factory=vae.sampler_net_factory(d, enc, H, H), hmc=hmc)
    dyn.generator = torch.Generator(device=dyn.device).manual_seed(5)
    aux = torch.as_tensor((np.random.RandomState(4).rand(n, n_pix) < 0.3).astype(np.float32)).cuda()
    return dyn, aux


def config5(n, hmc=False):
    """config 5's widths (latent 50, decoder 1024, 784 pixels, image branch 512, H = 200) on a two-step schedule"""
    return image_sampler(784, 50, 200, 512, 1024, n, T=2, hmc=hmc)


def train_sampler(composition, steps=STEPS, setup=None, MH=2, **shape):
    """`sampler_step` of the image sampler"""
    dyn, aux = image_sampler(**shape)
    if setup is not None:
        setup(dyn)
    tr = Trainer(dyn, decay_steps=0, seed=11)
    assert type(tr) is SplitTrainer and tr.image_sampler
    n, d = aux.shape[0], dyn.x_dim
    rng = np.random.RandomState(4)
    rng.rand(*aux.shape)                 # (the images were the first draws of this stream)
    log_sigma = torch.as_tensor((0.1 * rng.randn(n, d)).astype(np.float32)).cuda()
    x = start(d, n)
    for _ in range(steps):
        loss, x, _, _ = tr.sampler_step(x, aux, log_sigma, MH=MH, random_lf_composition=composition)
    return sha(tr.theta, tr.m, tr.v, x, np.float64(float(loss)))


def sample(dyn, n=N_CHAINS, n_proposals=3, aux=None):
    o = dyn.run(start(dyn.x_dim, n), None, 0, dyn.T, want=("x_next", "p", "x_hist"), n_proposals=n_proposals, rng=dict(seed=13), aux=aux)
    return sha(o["x_hist"], o["p"])


def sample_twice(dyn, aux):
    """two calls with the same images: the second finds the prepared weights and the image branch in the workspace (`reuse` = 3)"""
    first = sample(dyn, aux.shape[0], 1, aux)
    second = sample(dyn, aux.shape[0], 1, aux)
    assert dyn._last_reuse == 3, dyn._last_reuse
    return sha(np.frombuffer((first + second).encode(), np.uint8))


def hmc_both_ways(dyn, aux):
    x, v = start(dyn.x_dim, aux.shape[0]), torch.as_tensor(np.random.RandomState(6).randn(aux.shape[0], dyn.x_dim).astype(np.float32)).cuda()
    return sha(*(dyn.forward(x, init_v=v, aux=aux) + dyn.backward(x, init_v=v, aux=aux)))


def with_mode(pair_or_dyn, **attrs):
    for k, v in attrs.items():
        setattr(pair_or_dyn[0] if isinstance(pair_or_dyn, tuple) else pair_or_dyn, k, v)
    return pair_or_dyn


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


CASES = (
    ("train d<=4 kernel: SCG 2-d", lambda: train(dynamics(2, scg2d()), Trainer, Trainer)),
    ("train tile kernel: ICG 50-d", lambda: train(dynamics(50, icg(50)), Trainer, Trainer)),
    ("train raw precisions: mixture 2-d", lambda: train(dynamics(2, mog2d()), Trainer, Trainer)),
    ("train step-size override: ICG 50-d", lambda: train(stepped(dynamics(50, icg(50))), Trainer, Trainer)),
    ("train temperature 2.5: ICG 50-d", lambda: train(tempered(dynamics(50, icg(50))), Trainer, Trainer)),
    ("train LogisticTrainer: 32 rows, d = 8", lambda: train(dynamics(8, logistic()), LogisticTrainer, LogisticTrainer)),
    ("train GEMM engine, hess: dense 10-d, H = 32", lambda: train(dynamics(10, dense(10), H=32, T=5), Trainer, SplitTrainer)),
    ("train GEMM engine, energy + hvp callbacks: d = 3", lambda: train(dynamics(3, quadratic, T=5), Trainer, SplitTrainer)),
    ("train GEMM engine, net + vjp callbacks: d = 4", lambda: train(dynamics(4, icg(4), T=5, opaque=True), Trainer, SplitTrainer)),
    ("train image sampler, plain: MH = 2", lambda: train_sampler(0)),
    ("train image sampler, composed: R = 3", lambda: train_sampler(3)),
    ("sample fused engine: ICG 50-d", lambda: sample(dynamics(50, icg(50)))),
    ("sample GEMM engine, built-in: dense 10-d, H = 32", lambda: sample(dynamics(10, dense(10), H=32, T=5))),
    ("sample GEMM engine, callable energy: d = 3", lambda: sample(dynamics(3, quadratic, T=5))),
)

# `--engine`: every branch of the GEMM engine's host path (csrc/split.hip, csrc/train_split.hpp), each at the smallest shape that
# takes it -- the GEMM-engine cases above and the ones they leave out.  Run it against two builds of the LIBRARY (`L2HMC_LIB=`)
# with one version of the Python: the engine is bitwise reproducible, so a host-side change of it leaves every line as it was.
ENGINE_CASES = tuple(c for c in CASES if "GEMM engine" in c[0] or "image sampler" in c[0]) + (
    ("sample decoder posterior + image branch, twice (reuse = 3)", lambda: sample_twice(*image_sampler())),
    ("sample decoder posterior, HMC mode: forward and backward", lambda: hmc_both_ways(*image_sampler(hmc=True))),
    ("sample caller-supplied nets: d = 4", lambda: sample(dynamics(4, icg(4), T=5, opaque=True))),
    ("sample unfused nets (three products): d = 5, H = 18", lambda: sample(dynamics(5, dense(5), H=18, T=5))),
    ("sample 32 chains per workgroup: dense 10-d, H = 32, 32 x CUs chains", lambda: sample(dynamics(10, dense(10), H=32, T=5), 32 * cus(), 1)),
    ("sample planes, gemm_mode 1: config-5 widths, 3072 chains", lambda: sample_twice(*with_mode(config5(3072), gemm_mode=1))),
    ("sample planes, gemm_mode 3: config-5 widths, 3072 chains", lambda: sample_twice(*with_mode(config5(3072), gemm_mode=3))),
    ("sample in-loop split, gemm_mode 1: config-5 widths, 3071 chains", lambda: sample_twice(*with_mode(config5(3071), gemm_mode=1))),
    ("train three products per evaluation (net_mode 1): dense 10-d, H = 32",
     lambda: train(with_mode(dynamics(10, dense(10), H=32, T=5), net_mode=1), Trainer, SplitTrainer)),
    ("train unfused nets: d = 5, H = 18", lambda: train(dynamics(5, dense(5), H=18, T=5), Trainer, SplitTrainer)),
    ("train image sampler at temperature 2.5: one step, MH = 1", lambda: train_sampler(0, 1, tempered, MH=1)),
    ("train planes, gemm_mode 1: config-5 widths, 3072 chains, one step",
     lambda: train_sampler(0, 1, lambda dyn: with_mode(dyn, gemm_mode=1), n_pix=784, d=50, H=200, enc_hidden=512, dec_hidden=1024, n=3072, T=2)),
    ("train planes, gemm_mode 3: config-5 widths, 3072 chains, one step",
     lambda: train_sampler(0, 1, lambda dyn: with_mode(dyn, gemm_mode=3), n_pix=784, d=50, H=200, enc_hidden=512, dec_hidden=1024, n=3072, T=2)),
)


def host_time(warmup=20, calls=200):
    """`--host-time`: the launch-bound shape of the GEMM engine -- one synchronised `Dynamics.run` of the dense 10-d / H = 32 /
    T = 5 / 64-chain sampling case is ~25 short launches, so its wall time is the host side of the call"""
    import time
    dyn, x = dynamics(10, dense(10), H=32, T=5), start(10)
    v = torch.as_tensor(np.random.RandomState(6).randn(N_CHAINS, 10).astype(np.float32)).cuda()
    us = []
    for i in range(warmup + calls):
        t0 = time.perf_counter()
        dyn.run(x, v, 0, dyn.T)
        torch.cuda.synchronize()
        us.append(1e6 * (time.perf_counter() - t0))
    print("Dynamics.run dense 10-d, H = 32, T = 5, 64 chains: median %.1f us over %d synchronised calls after %d"
          % (float(np.median(us[warmup:])), calls, warmup), flush=True)


def main():
    torch.cuda.set_device(0)
    if "--host-time" in sys.argv[1:]:
        return host_time()
    for name, case in (ENGINE_CASES if "--engine" in sys.argv[1:] else CASES):
        print("%s  %s" % (case(), name), flush=True)


if __name__ == "__main__":
    main()
