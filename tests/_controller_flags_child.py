"""Run as a program, prints one digest per fixed script of tests/_controller_scripts.py (tests/_controller_drivers.py: `gpu_run`):

    XDE_CTRL_FLAGS=<flags> python -m tests._controller_flags_child

`XDE_CTRL_FLAGS` is read once per process (kernels and `xde_ctrl_wait` must agree on the publish protocol), so another protocol needs
a fresh process: tests/test_gpu_controller_kernels.py starts this module as a child, one at a time, and compares the digests with the
ones it computes in-process under the default flags ("all variants publish the same block").
"""
import os
import sys

import torch


def flags():
    return int(os.environ.get("XDE_CTRL_FLAGS", "15"))


def main():
    from paddlexde_amd import _hip

    from . import _controller_scripts as S
    from ._controller_drivers import digest, gpu_run

    be, dev = _hip.get_backend(), torch.device("cuda:0")
    checksummed = (flags() & 8) != 0
    for s0 in S.FIXED:
        for s in (s0, s0.reversed()):
            blocks, stages = gpu_run(be, dev, s, True)
            if not checksummed:  # nobody writes `chk`: it keeps what init left in it
                assert all(b.chk == 0 for b in blocks), s.id
            print("DIGEST", s.id, digest(s, blocks, stages), flush=True)
    torch.cuda.synchronize()
    print("CHILD OK flags={}".format(flags()), flush=True)


if __name__ == "__main__":
    sys.exit(main())
