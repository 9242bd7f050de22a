"""Drop-in for the two `chainer.serializers` calls the reference makes:
`save_hdf5(filename, obj)` and `load_hdf5(filename, obj)` (a3c.py:169-185,
demo_a3c_ale.py:61), for obj = a model (A3CModel) or its RMSpropAsync.

File layout = Chainer 1.8.1's HDF5Serializer on these objects:
  model:      one dataset per parameter at its link path, "0/0/W", "0/0/b",
              ... (pinned by trained_model/breakout_ff/80000000_finish.h5,
              tests/test_checkpoint.py);
  optimizer:  scalars "t" and "epoch", then every parameter's state under
              its path, "0/0/W/ms", ... (Optimizer.serialize restated; no
              reference .opt file exists to pin it); an Adam's states are
              "0/0/W/m", "0/0/W/v", ... and its "t" is the device's update
              count (DeviceNet.adam_t), written back on load.
Reading accepts the chunked/deflated files h5py writes; writing produces
contiguous datasets (hdf5.py).  Host-side, off the hot path."""
from __future__ import annotations

import numpy as np
import torch

from .hdf5 import read_hdf5, write_hdf5


def _is_optimizer(obj) -> bool:
    return hasattr(obj, "target") and hasattr(obj, "hooks")


def _is_adam(obj) -> bool:
    return hasattr(obj, "beta1") and hasattr(obj, "beta2")


def _states(obj, net):
    """(state name, flat device tensor) of the optimizer's per-parameter state:
    RMSpropAsync's ms, or Adam's m and v (v lives in the net's ms buffer)."""
    if _is_adam(obj):
        if net.adam_m is None:
            net.set_adam(obj.beta1, obj.beta2)
        return (("m", net.adam_m), ("v", net.ms))
    return (("ms", net.ms),)


def state_arrays(obj) -> dict:
    if _is_optimizer(obj):
        net = obj.target.net
        # Adam's update count is the device's: a graph replay moves it, not the host object's t
        t = net.adam_t() if _is_adam(obj) else int(getattr(obj, "t", 0))
        out = {"t": np.array(t, np.int64), "epoch": np.array(int(getattr(obj, "epoch", 0)), np.int64)}
        for state, flat in _states(obj, net):
            for name, a in net.state_dict(flat).items():
                out[name + "/" + state] = a
        return out
    return obj.net.state_dict()


def save_hdf5(filename, obj) -> None:
    """chainer.serializers.save_hdf5(filename, obj)."""
    write_hdf5(filename, state_arrays(obj))


def load_hdf5(filename, obj) -> None:
    """chainer.serializers.load_hdf5(filename, obj): every parameter (or
    optimizer state) of obj must be present with its shape; extra datasets
    are ignored, as Chainer's deserializer only visits obj's own entries."""
    data = read_hdf5(filename)
    if _is_optimizer(obj):
        net = obj.target.net
        obj.t = int(data["t"]) if "t" in data else 0
        obj.epoch = int(data["epoch"]) if "epoch" in data else 0
        for state, flat in _states(obj, net):
            for name, (_, shape) in net.layout.items():
                key = name + "/" + state
                if key not in data:
                    raise KeyError("%s: no dataset %s" % (filename, key))
                net.view(flat, name).copy_(torch.from_numpy(np.asarray(data[key], np.float32).reshape(shape)))
        if _is_adam(obj):
            net.set_adam_t(obj.t)
        return
    net = obj.net
    missing = [n for n in net.layout if n not in data]
    if missing:
        raise KeyError("%s: missing parameters %s" % (filename, missing))
    for name, (_, shape) in net.layout.items():
        if tuple(data[name].shape) != tuple(shape):
            raise ValueError("%s: %s has shape %s, model expects %s" % (filename, name, data[name].shape, shape))
    net.load_params({n: data[n] for n in net.layout})
