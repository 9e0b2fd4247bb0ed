import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


def _usable_cores():
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, min(n, 16))


def pytest_sessionstart(session):
    import torch
    if not torch.cuda.is_available():
        # the CPU tests compare the oracle with tests/golden/*.npz on host-independent code paths (oracle/pinned_cpu.py), set
        # before torch runs a kernel.  Not beside the GPU: the GPU parity bars were measured against the oracle's default paths.
        import pinned_cpu
        pinned_cpu.pin_env()
    torch.set_num_threads(_usable_cores())      # the CPU oracle must not oversubscribe a container with a CPU quota
