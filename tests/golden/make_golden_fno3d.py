#!/usr/bin/env python3
"""Capture golden vectors of the reference's 3D Fourier layer and FNO3d (CPU; run where the
reference checkout is available -- it never travels with the tests).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_fno3d.py --ref <reference checkout>

The reference's ``2d_FPE/FNOModules.py`` is imported in a subprocess (as make_golden.py does);
modules are seeded with torch.manual_seed, inputs and cotangents come from recipe.make_array.
Output: ``tests/golden/<case>.npz`` with ``in.x``, ``p.*``, ``out``, ``cot``, ``g.*``, ``gin.x``
(the two largest cases keep the backward arrays in ``<case>_bwd.npz``, see _save).
See tests/test_fno3d_golden.py and tests/test_gpu_fno3d.py for how they are used.
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# case -> (class, constructor arguments, input shape, torch seed)
CASES = {
    "sc3d_a": ("SpectralConv3d", (3, 4, 2, 3, 2), (2, 3, 8, 7, 9), 301),
    "sc3d_overlap": ("SpectralConv3d", (2, 3, 3, 3, 3), (2, 2, 5, 5, 8), 302),
    "sc3d_nyq": ("SpectralConv3d", (2, 2, 2, 2, 3), (2, 2, 6, 5, 4), 303),
    "sc3d_tiles": ("SpectralConv3d", (4, 4, 4, 4, 4), (2, 4, 18, 17, 19), 304),
    "fno3d_a": ("FNO3d", (3, 5, 4, 4, 2), (2, 6, 5, 7, 4), 305),
    "fno3d_b": ("FNO3d", (4, 8, 4, 3, 1), (2, 16, 15, 17, 3), 306),
}


def capture():
    import numpy as np
    import torch
    import FNOModules as FM
    from recipe import make_array

    for name, (cls, args, shape, seed) in CASES.items():
        torch.manual_seed(seed)
        m = getattr(FM, cls)(*args)
        x = torch.from_numpy(make_array(shape, seed, name + ".x")).requires_grad_(True)
        out = m(x)
        cot = torch.from_numpy(make_array(tuple(out.shape), seed, name + ".cot"))
        (out * cot).sum().backward()
        arr = {"in.x": x.detach().numpy(), "out": out.detach().numpy(), "cot": cot.numpy(),
               "gin.x": x.grad.numpy()}
        for k, v in m.state_dict().items():
            arr["p." + k] = v.detach().numpy()
        for k, p in m.named_parameters():
            arr["g." + k] = p.grad.numpy()
        _save(name, arr)


SPLIT_BYTES = 512 * 1024


def _save(name, arr):
    """One ``<name>.npz``; a case past SPLIT_BYTES (random fp32 data does not compress) goes into
    ``<name>.npz`` (in.x, p.*, out) and ``<name>_bwd.npz`` (cot, g.*, gin.x), so that no committed
    file nears the repository's 1 MiB limit.  The tests merge the two."""
    import numpy as np

    def write(n, a):
        path = os.path.join(HERE, f"{n}.npz")
        np.savez_compressed(path, **a)
        print(f"  wrote {n}.npz ({os.path.getsize(path) / 1024:.1f} KiB, {len(a)} arrays)")

    if sum(v.nbytes for v in arr.values()) <= SPLIT_BYTES:
        write(name, arr)
        return
    bwd = {k: v for k, v in arr.items() if k == "cot" or k.startswith(("g.", "gin."))}
    write(name, {k: v for k, v in arr.items() if k not in bwd})
    write(name + "_bwd", bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference repository")
    ap.add_argument("--capture", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.capture:
        sys.path.insert(0, os.path.join(a.ref, "2d_FPE"))
        capture()
        return
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, __file__, "--ref", a.ref, "--capture"], check=True, env=env)


if __name__ == "__main__":
    main()
