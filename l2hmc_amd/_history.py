"""The host side of a statistics call on a recorded history (steps, chains, dim), said once for `func_utils`, `diagnostics`,
`quantiles`, `multivariate` and `predictive`: which inputs go to the HIP kernels, how a device history is read where it lies,
how a launch is made on the history's own device, how host data becomes numpy, and which shapes are refused.  A ROCm tensor
goes to the kernels and only a few sums come back; numpy or a CPU tensor is host arithmetic (there is no CPU path for
sampling, but statistics of host data are computed on the host).  `import torch` stays lazy: numpy input needs no torch."""
import numpy as np

from . import _ffi


def is_device_tensor(X):
    try:
        import torch
        return isinstance(X, torch.Tensor) and X.is_cuda
    except ImportError:
        return False


def in_place(X):
    """The float32 contiguous tensor a kernel reads: X itself when it already is one (a first-axis slice of a history -- a
    burn-in cut -- is contiguous and is not copied), else the converted copy.  Always on the device of X."""
    import torch
    X = X.detach()
    if X.dtype != torch.float32 or not X.is_contiguous():
        X = X.to(torch.float32).contiguous()
    return X


def as_numpy(a, dtype=None):
    """A torch tensor (detached, brought to the host when it is not there) or anything numpy takes, as a numpy array."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=dtype)


def launch(dev, fn, *args):
    """`fn(*args, stream)` with `dev` the current device and `stream` its current stream; the checked return code."""
    import torch
    with torch.cuda.device(dev):
        return _ffi.check(fn(*args, _ffi.current_stream(dev)))


def workspace(dev, dtype, query, *args, at_least=0):
    """`query(*args)` elements (never fewer than `at_least`) of `dtype` on `dev`."""
    import torch
    return torch.empty(max(at_least, _ffi.check(query(*args))), dtype=dtype, device=dev)


def history_shape(X, flat_ok=False, says=None):
    """The shape of X as ints when it is a history (steps, chains, dim) -- or, with `flat_ok`, (draws, dim); ValueError
    otherwise, opening with `says` where a caller words the refusal itself."""
    shape = tuple(int(v) for v in X.shape)
    if len(shape) != 3 and not (flat_ok and len(shape) == 2):
        raise ValueError("%s; got shape %s" % (says or "a history is (steps, chains, dim)" + (" or (draws, dim)" if flat_ok else ""),
                                               shape))
    return shape
