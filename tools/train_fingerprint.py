#!/usr/bin/env python
"""Bit-for-bit fingerprint of the host side of training and sampling (GPU box): one SHA-256 per code path of the Python that
marshals a launch, each case at the smallest shape that still takes its path.  Public API only, so the same file runs against
two versions of `l2hmc_amd/*.py` on ONE build of the library (`L2HMC_LIB=`): a host-side refactor must leave every line as it
was.

    python tools/train_fingerprint.py

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


def train_sampler(composition):
    """the image-conditioned sampler of the VAE experiment: 16 pixels, latent 4, hidden 8, 32 chains, MH = 2"""
    seeded()
    n_pix, d, H, n = 16, 4, 8, 32
    enc = vae.make_encoder_sampler(n_pix, H, H)
    dyn = Dynamics(d, vae.VAEPosterior(vae.make_decoder(d, H, n_pix)).get_energy_function(), T=5, eps=0.1,
                   net_factory=vae.sampler_net_factory(d, enc, H, H))
    dyn.generator = torch.Generator(device=dyn.device).manual_seed(5)
    tr = Trainer(dyn, decay_steps=0, seed=11)
    assert type(tr) is SplitTrainer and tr.image_sampler
    rng = np.random.RandomState(4)
    aux = torch.as_tensor((rng.rand(n, n_pix) < 0.3).astype(np.float32)).cuda()
    log_sigma = torch.as_tensor((0.1 * rng.randn(n, d)).astype(np.float32)).cuda()
    x = start(d, n)
    for _ in range(STEPS):
        loss, x, _, _ = tr.sampler_step(x, aux, log_sigma, MH=2, random_lf_composition=composition)
    return sha(tr.theta, tr.m, tr.v, x, np.float64(float(loss)))


def sample(dyn):
    o = dyn.run(start(dyn.x_dim), None, 0, dyn.T, want=("x_next", "p", "x_hist"), n_proposals=3, rng=dict(seed=13))
    return sha(o["x_hist"], o["p"])


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


def main():
    torch.cuda.set_device(0)
    for name, case in CASES:
        print("%s  %s" % (case(), name), flush=True)


if __name__ == "__main__":
    main()
