"""numpy / int restatement of the device k-means++ initialisation
(include/vqgnn.h §12, csrc/kmeans_kernels.hip).  TEST INFRASTRUCTURE ONLY.

The stream is oracle/subgraph_ref.walk_mix; the distance is the arithmetic of
oracle/vq_ref.py's ``distances`` as the golden fixtures pin it
(tests/helpers.sequential_argmin): |z|^2 and |c|^2 summed sequentially in
fp32, z.c a k-ordered fp32 fma chain from fl(z0 c0), d = fl(fl(|z|^2 + |c|^2)
- 2 z.c); every fp32 operation below is a single correct rounding.  Weights
and prefix sums are integers.
"""
import math

import numpy as np

from oracle.subgraph_ref import walk_mix

_M64 = (1 << 64) - 1
F32 = np.float32


def fma32(a, b, c):
    """fl32(a * b + c) with one rounding, elementwise.  The product of two
    fp32 values is exact in fp64; the fp64 sum is turned into round-to-odd
    with its TwoSum error, which makes the final fp32 rounding correct."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = np.ascontiguousarray(s).view(np.int64).copy()
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)
    away = (err > 0) == (s > 0)
    bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
    return bits.view(np.float64).astype(F32)


def normalise(X, coef, b, D, W=None):
    """Branch b's points: fma(x - shift, alpha, beta) with coef [6, nb*D]."""
    W = D if W is None else W
    X = np.asarray(X, F32)
    F = coef.shape[1]
    assert coef.shape[0] == 6 and F % D == 0
    cols = slice(b * D, b * D + W)
    t = X[:, cols] - coef[4, cols].astype(F32)[None]          # one fp32 rounding
    return fma32(t, coef[0, cols][None], coef[1, cols][None])


def sumsq(v):
    """Sequential fp32 sum of squares over the last axis (separate mul, add)."""
    v = np.asarray(v, F32)
    s = v[..., 0] * v[..., 0]
    for k in range(1, v.shape[-1]):
        s = (s + v[..., k] * v[..., k]).astype(F32)
    return s.astype(F32)


def distances(z, c):
    """d[i, m] for points z [n, W] and centroids c [M, W]."""
    z, c = np.asarray(z, F32), np.asarray(c, F32)
    zz, cc = sumsq(z)[:, None], sumsq(c)[None, :]
    dot = (z[:, None, 0] * c[None, :, 0]).astype(F32)
    for k in range(1, z.shape[1]):
        dot = fma32(z[:, None, k], c[None, :, k], dot)
    return fma32(F32(-2.0), dot, (zz + cc).astype(F32))


def draw(seed, b, s):
    """r(b, s) = mix(mix(seed ^ mix(b)) + s), all 64 bits."""
    return walk_mix((walk_mix((seed & _M64) ^ walk_mix(b)) + s) & _M64)


def weights(mind):
    """q = llrint(min(mind, 2^20) * 2^20) as int64 (exact product, ties to even)."""
    return np.rint(np.minimum(mind, F32(2.0 ** 20)).astype(np.float64) * 2.0 ** 20).astype(np.int64)


def seed_branch(z, M, seed, b):
    """-> (seed_rows [M] int32, centroids [M, W] f32, steps that met T = 0)."""
    z = np.asarray(z, F32)
    B = z.shape[0]
    rows = np.empty(M, np.int32)
    mind = np.full(B, np.inf, F32)
    zero_steps = 0
    for s in range(M):
        r = draw(seed, b, s)
        if s == 0:
            i = r % B
        else:
            q = [int(v) for v in weights(mind)]
            T = sum(q)
            if T == 0:
                zero_steps += 1
                i = r % B
            else:
                t, acc, i = r % T, 0, -1
                for j, v in enumerate(q):
                    acc += v
                    if acc > t:
                        i = j
                        break
        rows[s] = i
        d = distances(z, z[i:i + 1])[:, 0]
        mind = np.minimum(mind, np.maximum(d, F32(0.0))).astype(F32)
        mind[i] = 0.0
    return rows, z[rows].copy(), zero_steps


def stat_shift(count):
    """vqgnn_vq_stat_shifts(count, 1)'s feature shift: |z| <= sqrt(count) < 2^e."""
    e = math.frexp(math.sqrt(max(int(count), 1)))[1]
    return 30 - e


def assign(z, c):
    """First-index argmin labels [n] int64."""
    return np.argmin(distances(z, c), axis=1).astype(np.int64)


def lloyd_step(z, c, labels, shift):
    """Counts [M] int64 and the updated centroids: c_k = (float)((double)S_k *
    2^-shift / (double)n) with S_k the sum of rint(z_k * 2^shift); empty
    clusters keep their centroid."""
    z = np.asarray(z, F32)
    M = c.shape[0]
    fixed = np.rint(np.ldexp(z.astype(np.float64), shift)).astype(np.int64)
    counts = np.bincount(labels, minlength=M).astype(np.int64)
    out = np.array(c, F32, copy=True)
    for m in np.nonzero(counts)[0]:
        S = fixed[labels == m].sum(axis=0)
        out[m] = (np.ldexp(S.astype(np.float64), -shift) / float(counts[m])).astype(F32)
    return counts, out


def fit_branch(z, M, iters, seed, b, stat_count=None):
    """The whole fit of one branch -> dict(seed_rows, seeds, centroids [iters
    + 1 entries: the centroids each assign ran against], labels [per assign],
    counts [per assign])."""
    shift = stat_shift(z.shape[0] if stat_count is None else stat_count)
    rows, c, zero_steps = seed_branch(z, M, seed, b)
    out = dict(seed_rows=rows, seeds=c.copy(), zero_steps=zero_steps, centroids=[], labels=[],
               counts=[])
    for it in range(iters + 1):
        lab = assign(z, c)
        counts, nxt = lloyd_step(z, c, lab, shift)
        out["centroids"].append(c.copy())
        out["labels"].append(lab)
        out["counts"].append(counts)
        if it < iters:
            c = nxt
    return out
