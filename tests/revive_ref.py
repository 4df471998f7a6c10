"""numpy / int restatement of the dead-codeword revival (include/vqgnn.h §13,
csrc/kmeans_kernels.hip).  TEST INFRASTRUCTURE ONLY.

The points, the distance, the weights and the draw are tests/kmeans_ref.py's
(§12); every fp32 operation below is a single correct rounding, the weights
and prefix sums are integers.
"""
import numpy as np

from kmeans_ref import F32, distances, draw, fma32, normalise, weights  # noqa: F401

from oracle.subgraph_ref import walk_mix

_M64 = (1 << 64) - 1


def layer_seed(kmeans_seed, call_number):
    """The seed of a layer's revival after its call_number-th batched VQ call:
    mix(kmeans_seed ^ mix(call_number)), mix = §9b's splitmix64 finaliser."""
    return walk_mix((kmeans_seed & _M64) ^ walk_mix(call_number))


def initial_mind(z, emb_f, labels):
    """mind_i = max(d(z_i, emb_f[labels_i]), 0); 0 for a label outside [0, M)."""
    z, emb_f = np.asarray(z, F32), np.asarray(emb_f, F32)
    labels = np.asarray(labels, np.int64)
    ok = (labels >= 0) & (labels < emb_f.shape[0])
    mind = np.zeros(z.shape[0], F32)
    d = distances(z, emb_f)
    idx = np.nonzero(ok)[0]
    mind[idx] = np.maximum(d[idx, labels[idx]], F32(0.0))
    return mind


def nearest_mind(z, emb_f):
    """max(min_m d(z_i, emb_f[m]), 0) per row: the quantisation error the D^2
    step samples from when the labels are the argmin."""
    return np.maximum(distances(z, emb_f).min(axis=1), F32(0.0)).astype(F32)


def pick(mind, r):
    """§12's draw -> (row, T == 0)."""
    cum = np.cumsum(weights(mind))          # <= 2^23 rows * 2^40: exact in int64
    T = int(cum[-1])
    if T == 0:
        return r % mind.shape[0], True
    return int(np.searchsorted(cum, r % T, side="right")), False


def revive_branch(z, b, cs, emb, ema_w, emb_out, labels, rm, rv, threshold, R, init_count, seed):
    """Branch b in place on cs [M], emb / ema_w / emb_out [M, ldw] (ldw = D or
    >= 2D), with z [B, D] its points, rm / rv [D] its running statistics.
    -> (n_slots, slots [R] int32, rows [R] int32, steps that met T = 0)."""
    z = np.asarray(z, F32)
    D, ldw = z.shape[1], emb.shape[1]
    thr, ic = F32(threshold), F32(init_count)
    dead = np.nonzero(cs < thr)[0]                   # a NaN is not dead
    n = min(dead.shape[0], R)
    slots = np.full(R, -1, np.int32)
    slots[:n] = dead[:n]
    rows = np.full(R, -1, np.int32)
    mind = initial_mind(z, emb[:, :D], labels)
    sd = np.sqrt((rv + F32(1e-5)).astype(F32)).astype(F32)
    zero_steps = 0
    for s in range(n):
        i, zero = pick(mind, draw(seed, b, s))
        zero_steps += zero
        m = slots[s]
        rows[s] = i
        emb[m, :D] = z[i]
        cs[m] = ic
        ema_w[m, :D] = (z[i] * ic).astype(F32)
        if ldw >= 2 * D:
            ema_w[m, D:2 * D] = (emb[m, D:2 * D] * ic).astype(F32)
        emb_out[m, :D] = ((z[i] * sd).astype(F32) + rm).astype(F32)
        d = distances(z, z[i:i + 1])[:, 0]
        mind = np.minimum(mind, np.maximum(d, F32(0.0))).astype(F32)
        mind[i] = 0.0
    return n, slots, rows, zero_steps


def revive(X, coef, D, state, labels, threshold, R, init_count, seed, codes=None, batch_idx=None):
    """All branches.  state: dict(cs [nb, M], emb, ema_w, emb_out [nb, M, ldw],
    rm_f, rv_f [nb, D]) of float32 arrays; labels [nb, B] int64.  -> dict of
    the state after the call (copies) + n_slots [nb], slots, rows [nb, R],
    zero_steps and, when given, the codes [N, >= nb] int16 after the scatter."""
    out = {k: np.array(state[k], F32, copy=True) for k in ("cs", "emb", "ema_w", "emb_out")}
    nb = out["cs"].shape[0]
    out["n_slots"] = np.zeros(nb, np.int32)
    out["slots"] = np.full((nb, R), -1, np.int32)
    out["rows"] = np.full((nb, R), -1, np.int32)
    out["zero_steps"] = 0
    if codes is not None:
        out["codes"] = np.array(codes, np.int16, copy=True)
    for b in range(nb):
        z = normalise(X, coef, b, D)
        n, slots, rows, zs = revive_branch(z, b, out["cs"][b], out["emb"][b], out["ema_w"][b],
                                           out["emb_out"][b], labels[b], state["rm_f"][b],
                                           state["rv_f"][b], threshold, R, init_count, seed)
        out["n_slots"][b], out["slots"][b], out["rows"][b] = n, slots, rows
        out["zero_steps"] += zs
        if codes is not None:
            for s in range(n):
                out["codes"][batch_idx[rows[s]], b] = slots[s]
    return out
