"""Host-independent CPU arithmetic for the oracle's golden comparisons (test infrastructure).

The golden vectors (tests/golden/*.npz) are the reference's outputs; the tests recompute them with the oracle and compare at
f32 tolerances.  PyTorch's CPU kernels pick their code path from the host's instruction set (ATen's vectorised loops, MKL's
GEMM branch, oneDNN's JIT convolutions), and each path sums in another order: over a few Adam steps at beta1 = 0 that
difference alone exceeds those tolerances.  So both sides run on paths every x86-64 host executes alike: ATen's scalar
kernels, MKL's reproducible COMPATIBLE branch and PyTorch's own convolutions instead of oneDNN's, on a fixed thread count.

`pin_env()` must run before torch executes its first kernel (ATen and MKL read the variables once); `no_onednn()` is a
context manager for the code that compares against the goldens."""
import contextlib
import os

ENV = {"ATEN_CPU_CAPABILITY": "default", "MKL_CBWR": "COMPATIBLE", "ONEDNN_MAX_CPU_ISA": "SSE41"}
THREADS = 4


def pin_env():
    os.environ.update(ENV)


@contextlib.contextmanager
def no_onednn():
    import torch
    was = torch.backends.mkldnn.enabled
    torch.backends.mkldnn.enabled = False
    try:
        yield
    finally:
        torch.backends.mkldnn.enabled = was
