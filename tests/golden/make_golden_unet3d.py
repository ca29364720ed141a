"""Writes tests/golden/layouts_unet3d.json: names / shapes / dtypes of PermInvUNet_attn3D's
state_dict, spelled out from plain torch.nn modules in the 2D class's creation order
(2d_FPE/NIOModules.py:1086-1181 carried to three axes) -- independently of blindno/unet3d.py,
which tests/test_unet3d_ref.py compares with it.  The head is the project's FNO3d.

    python tests/golden/make_golden_unet3d.py
"""
from __future__ import annotations

import json
import os
import sys

import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "reconstruction-of-pde-without-time-label_amd"))

CONFIGS = {
    "PermInvUNet_attn3D(1,2,1,3,(40,40,40))": dict(base_ch=1, depth=3, input_size=(40, 40, 40), width=8, modes=4),
    "PermInvUNet_attn3D(1,2,2,2,(9,12,10),width=4,modes=2)": dict(base_ch=2, depth=2, input_size=(9, 12, 10),
                                                                   width=4, modes=2),
}


def cnx(dim):
    return nn.ModuleDict(dict(dwconv=nn.Conv3d(dim, dim, 7, padding=3, groups=dim), norm=nn.LayerNorm(dim, eps=1e-6),
                              pwconv1=nn.Linear(dim, 4 * dim), act=nn.GELU(), pwconv2=nn.Linear(4 * dim, dim)))


def att(n):
    return nn.ModuleDict(dict(norm=nn.LayerNorm(n)))


def build(base_ch, depth, input_size, width, modes, in_ch=1, out_ch=2):
    from blindno.fno import FNO3d
    chs = [base_ch * 2 ** i for i in range(depth + 1)]
    sizes = [[n] for n in input_size]
    for s in sizes:
        for _ in range(depth):
            s.append(s[-1] // 2)
    m = nn.Module()
    m.down_convs = nn.ModuleList([nn.Sequential(nn.Conv3d(in_ch, chs[0], 3, padding=1), cnx(chs[0]))])
    m.pools = nn.ModuleList()
    for i in range(depth):
        m.pools.append(nn.MaxPool3d(2))
        m.down_convs.append(nn.Sequential(nn.Conv3d(chs[i], chs[i + 1], 3, padding=1), cnx(chs[i + 1])))
    m.skip_norms = nn.ModuleList([nn.BatchNorm3d(c) for c in chs])
    m.temp_atts = nn.ModuleList([att(chs[i] * sizes[0][i] * sizes[1][i] * sizes[2][i]) for i in range(depth + 1)])
    m.up_transposes = nn.ModuleList()
    m.up_convs = nn.ModuleList()
    for i in reversed(range(depth)):
        m.up_transposes.append(nn.ConvTranspose3d(chs[i + 1], chs[i], 2, stride=2))
        m.up_convs.append(nn.Sequential(nn.Conv3d(2 * chs[i], chs[i], 3, padding=1), cnx(chs[i])))
    m.final_conv = nn.Conv3d(chs[0], width, 1)
    m.fno = FNO3d(modes, width, 2, width, out_ch)
    return m


def layout(m):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in m.state_dict().items()]


if __name__ == "__main__":
    with open(os.path.join(HERE, "layouts_unet3d.json"), "w") as f:
        json.dump({k: layout(build(**c)) for k, c in CONFIGS.items()}, f, indent=0)
    print("wrote layouts_unet3d.json")
