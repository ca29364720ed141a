"""The cases of the NIOFP2D_attn coefficient-attention tests (tests/test_nio2d_attn.py on the CPU,
tests/test_gpu_nioattn.py on the device): shapes, logit regimes and their inputs, with the regime
asserted on the float64 restatement nio2d_attn_ref.attn_math.

Tokens of this model have rank <= Q = P + 3: token 2 + l is (w_l . basis + b0) / sqrt(P), so with
basis ~ N(0, 1) and w ~ a N(0, 1) a token has standard deviation a, its diagonal logit is about
a^2 sqrt(S), and the off-diagonal logits are about a^2 sqrt(S / P) N(0, 1): larger than those of
independent tokens (a^2 N(0, 1), tests/test_gpu_bagagg.py) by sqrt(S / P).  The grid tokens are
drawn at the same amplitude (any (S, 2) values will do for the kernels).  Found on the CPU: a
diagonal logit of 0.1 keeps every |logit| <= 1 on all shapes (0.2 does not: 1.03 at P = 7), log T puts the mean row
maximum of A in [0.2, 0.8] with a softmax share of dw of 14 % or more, T = 3 included, and 220 gives a
largest logit of 340 or more.  No (shape, regime) pair is skipped.
"""
import functools
import math

import torch

import nio2d_attn_ref

# B, L, S, P, width: the smallest shapes at which each mechanism of csrc/nioattn.hip can fail
SHAPES = [
    (2, 1, 25, 1, 1),        # T = 3, Q = 4, S below one wave
    (3, 5, 63, 25, 5),       # T not a multiple of 4 (a wave without a row in the last round), S < 64
    (2, 12, 1023, 25, 3),    # eight moment partials and backward blocks with a ragged 127-point tail
    (2, 30, 513, 7, 4),      # a one-point tail in both the moments and the backward passes
    (1, 254, 64, 64, 2),     # both caps: T = 256, Q = 67, largest LDS
    (2, 53, 512, 25, 20),    # wide output
    (70, 3, 64, 25, 2),      # more bags than a chunk of 64
]
REGIMES = ("diffuse", "mixed", "sharp")


def diagonal_logit(regime, L):
    return {"diffuse": 0.1, "mixed": math.log(L + 2), "sharp": 220.0}[regime]


def inputs_of(B, L, S, P, width, regime, seed=None):
    gen = torch.Generator().manual_seed(1000 * S + 10 * L + REGIMES.index(regime) if seed is None else seed)
    a = math.sqrt(diagonal_logit(regime, L) / math.sqrt(S))
    grid = a * torch.randn(S, 2, generator=gen)
    basis = torch.randn(S, P, generator=gen)
    w = a * torch.randn(B, L, P, generator=gen)
    b0 = (0.1 * a * torch.randn(1, generator=gen)).reshape(())
    fc0w = torch.randn(width, generator=gen)
    fc0b = torch.randn(width, generator=gen)
    dy = torch.randn(B, S, width, generator=gen)
    return (w, basis, b0, grid, fc0w, fc0b, dy)


@functools.lru_cache(maxsize=None)
def make_case(B, L, S, P, width, regime):
    """(fp32 host inputs, float64 attn_math of them); the regime is asserted here."""
    inputs = inputs_of(B, L, S, P, width, regime)
    ref = nio2d_attn_ref.attn_math(*inputs, torch.float64)
    logits = ref["logits"]
    rowmax = float(ref["A"].max(-1).values.mean())
    share = float(torch.linalg.vector_norm(ref["soft_w"]) / torch.linalg.vector_norm(ref["dw"]))
    print(f"nioattn B={B} L={L} S={S} P={P} width={width} {regime}: max |logit| "
          f"{float(logits.abs().max()):.3g}, mean row max of A {rowmax:.3f}, softmax share of dw {share:.3%}")
    if regime == "diffuse":
        assert float(logits.abs().max()) <= 1.0
    elif regime == "mixed":
        assert 0.2 <= rowmax <= 0.8
        assert share >= 0.02
    else:
        assert float(logits.max()) >= 150.0
    return inputs, ref
