"""Run as a program, prints one digest per case of tests/_seam_drivers.py (`state_machine`, `carry_run`):

    XDE_NT=0 python -m tests._seam_nt_child

`XDE_NT` (the load policy of the combine / error-norm kernels, csrc/xde_common.hpp) is read once per process, and bit 0 of it selects
between the two instantiations of `xde_seam_kernel` per dtype and norm: the ones with plain loads need a fresh process.
tests/test_gpu_seam_kernel.py starts this module as a child and compares the digests with the ones it computes in-process under the
default policy.  Every case runs with its own assertions (against the numpy double, against the three launches) here too.
"""
import os
import sys

import torch

# (a) at n = 3077 for both state and time dtypes; (b) at 1 and 5 vectors per lane for both dtypes and both norms
CASES = [("a", sdt, tdt, 3077) for sdt in ("f32", "f64") for tdt in ("f64", "f32")] + \
        [("b", sdt, norm, p) for sdt in ("f32", "f64") for norm in ("rms", "linf") for p in (5, 1)]


def nt():
    return int(os.environ.get("XDE_NT", "7"))


def main():
    from paddlexde_amd import _hip

    from . import _seam_drivers as D
    from ._seam_double import SeamDoubleBackend

    be, dbl, dev = _hip.get_backend(), SeamDoubleBackend(), torch.device("cuda:0")
    ws = be.new_workspace(dev), be.new_workspace(dev)
    for key in CASES:
        if key[0] == "a":
            d = D.state_machine(be, dbl, dev, key[1], key[2], key[3])
        else:
            d = D.carry_run(be, dev, key[1], key[2], key[3], *ws)
        print("DIGEST", "-".join(map(str, key)), d, flush=True)
    torch.cuda.synchronize()
    print("CHILD OK nt={}".format(nt()), flush=True)


if __name__ == "__main__":
    sys.exit(main())
