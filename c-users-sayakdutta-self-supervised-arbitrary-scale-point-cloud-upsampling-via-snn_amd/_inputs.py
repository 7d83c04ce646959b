"""The input checks of the evaluation modules (metrics, mesh, ray, normals, sinkhorn, surface, data), in one place.

An [n,3] input is a numpy array or a device tensor of any float dtype, contiguous or not.  ``checked`` is everything that can be
said about one on the host; ``upload`` makes contiguous f64 tensors on one device; ``on_device`` is the usual sequence of the two.
A numpy input is tested for NaN / infinity on the host, before the upload, and a device tensor on the device, after it: each once.
``device_tensor`` is the check of an input that has to be a device tensor already.  Every output of this module is a converted
input: nothing here allocates a buffer for a kernel to fill.
"""
import numpy as np
import torch


def checked(x, name, min_rows=0, finite=False):
    """One [n,3] input after its host checks, in this order: shape, dtype, placement (a CPU tensor is refused: there is no CPU
    path), at least ``min_rows`` rows, and with ``finite`` no NaN or infinity in a numpy array (a device tensor's values are
    ``finite_on_device``'s to test).  Returns the tensor, or the input as a numpy array."""
    if torch.is_tensor(x):
        shape, on_host, floating = tuple(x.shape), not x.is_cuda, x.dtype.is_floating_point
    else:
        x = np.asarray(x)
        shape, on_host, floating = x.shape, False, x.dtype.kind == "f"
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("%s: expected points [n, 3], got shape %s" % (name, tuple(shape)))
    if not floating:
        raise ValueError("%s: expected a floating dtype" % name)
    if on_host:
        raise RuntimeError("%s: a CPU tensor (there is no CPU path; pass a device tensor or a numpy array)" % name)
    if shape[0] < min_rows:
        raise ValueError("%s: an empty cloud" % name)
    if finite and not torch.is_tensor(x) and not np.isfinite(x).all():
        raise ValueError("%s contains NaN or infinity" % name)
    return x


def upload(xs, device=None, others=()):
    """The checked inputs ``xs`` as contiguous f64 tensors on one device: ``device``, else that of the first tensor among ``xs`` and
    ``others``, else the current one."""
    if device is None:
        device = next((t.device for t in tuple(xs) + tuple(others) if torch.is_tensor(t)), None)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    out = []
    for x in xs:
        if not torch.is_tensor(x):
            x = np.ascontiguousarray(x, dtype=np.float64)
            x = torch.from_numpy(x if x.flags.writeable else x.copy())
        out.append(x.to(device=device, dtype=torch.float64).contiguous())
    return out


def finite_on_device(xs, uploaded, names):
    """ValueError for the first of the inputs ``xs`` that came as a device tensor and holds a NaN or an infinity (one
    synchronisation per tensor); ``uploaded`` are their f64 copies."""
    for x, t, name in zip(xs, uploaded, names):
        if torch.is_tensor(x) and not bool(torch.isfinite(t).all()):
            raise ValueError("%s contains NaN or infinity" % name)


def on_device(inputs, device=None, min_rows=0, finite=False):
    """``inputs``, a sequence of (x, name), as contiguous f64 [n,3] tensors on one device (``upload``'s choice).  Shape, dtype and
    placement of every input are checked first, then the row count (``min_rows``: one number, or one per input) and, with
    ``finite``, the values of every numpy input, all before anything is uploaded; the device tensors' values after it."""
    rows = min_rows if isinstance(min_rows, tuple) else (min_rows,) * len(inputs)
    for x, name in inputs:
        checked(x, name)
    xs = [checked(x, name, r, finite) for (x, name), r in zip(inputs, rows)]
    out = upload(xs, device)
    if finite:
        finite_on_device(xs, out, [name for _, name in inputs])
    return out


def device_tensor(dev, owner, t, name, dtype, shape, optional=False):
    """``t`` as a contiguous ``dtype`` tensor: it has to be a device tensor of the shape ``shape`` (None: any extent) on ``dev``, the
    device of ``owner`` ("the tables", "the clouds"), floating or integer as ``dtype`` is.  ``optional``: None stays None.  The
    first two arguments are the caller's to bind once (``functools.partial``)."""
    if t is None and optional:
        return None
    if not torch.is_tensor(t):
        raise ValueError("%s: expected a device tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s: a CPU tensor (there is no CPU path)" % name)
    if t.dim() != len(shape) or any(w is not None and s != w for s, w in zip(t.shape, shape)):
        raise ValueError("%s: expected shape %s, got %s" % (name, list(shape), list(t.shape)))
    if t.device != dev:
        raise ValueError("%s: on %s, %s are on %s" % (name, t.device, owner, dev))
    if dtype.is_floating_point != t.dtype.is_floating_point:
        raise ValueError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    return t.to(dtype).contiguous()
