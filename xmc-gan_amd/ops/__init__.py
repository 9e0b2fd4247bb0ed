"""Autograd-visible operators backed by libxmc_gan_hip.so.

Every operator is a ``torch.autograd.Function`` whose backward is itself written with operators
from this package, so the set is closed under differentiation: that is what lets the MA-GP term
(train_gan.py:231-252, ``autograd.grad(create_graph=True)`` followed by ``backward()``) run through
hand-written kernels.  Activations are contiguous NHWC tensors ``[N,H,W,C]`` (C % 8 == 0) in the
engine's activation dtype (bf16 by default, f32 in parity mode); parameters stay f32 in the
reference's ``[Co,Ci,KH,KW]`` / ``[out,in]`` layout and are packed on demand (cached).
PyTorch is used for storage, streams and the autograd graph only.

The modules are layers: each imports only from those before it in the tuple below.
"""
from types import ModuleType
from . import _config, _engine, _forward, _nodes_leaf, _nodes_conv, _nodes_block, _nodes_loss, _functional

# the public (and test-visible) surface: everything the modules define, under its own name
for _m in (_config, _engine, _forward, _nodes_leaf, _nodes_conv, _nodes_block, _nodes_loss, _functional):
    globals().update({_k: _v for _k, _v in vars(_m).items() if not _k.startswith("__") and not isinstance(_v, ModuleType)})
del _m, ModuleType
