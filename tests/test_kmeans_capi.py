"""C-ABI of the device k-means++ initialisation (include/vqgnn.h §12): the
entries exist and are bound, reject bad arguments before any launch, and the
host wrappers refuse CPU tensors.  No GPU here: every pointer below is a dummy
address that validation never dereferences."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import vq_gnn_amd._lib as L
from vq_gnn_amd import kernels
from vq_gnn_amd.vq import VQBank

import kmeans_ref

P = 4096      # dummy non-null device address


def _seed(X=P, ldx=16, B=100, nb=4, D=4, M=16, W=4, coef=P, seed=0, cent=P, ldw=4, bstride=None,
          rows=P, ws=P):
    h = L.lib()
    bstride = M * ldw if bstride is None else bstride
    rc = h.vqgnn_kmeans_seed(X, ldx, B, nb, D, M, W, coef, seed, cent, ldw, bstride, rows, ws, None)
    return rc, h.vqgnn_last_error()


def test_entries_exist_and_are_bound():
    h = L.lib()
    for name in ("vqgnn_kmeans_workspace", "vqgnn_kmeans_seed", "vqgnn_kmeans_centroids"):
        assert name in L.SIGNATURES
        fn = getattr(h, name)
        assert fn.argtypes == L.SIGNATURES[name][1]
    for name in ("kmeans_seed", "kmeans_centroids"):
        assert callable(getattr(kernels, name))
    assert callable(VQBank.kmeans_fit)


@pytest.mark.parametrize("kw,text", [
    (dict(X=None), b"null"),
    (dict(coef=None), b"null"),
    (dict(cent=None), b"null"),
    (dict(rows=None), b"null"),
    (dict(ws=None), b"null"),
    (dict(M=101), b"M=101"),                       # M > B
    (dict(W=9, D=9, ldx=36, ldw=9), b"W=9"),       # W > 8
    (dict(B=(1 << 23) + 1, M=16, ldx=16), b"2^23"),
    (dict(B=40000, M=32768), b"int16"),            # M outside int16 range
    (dict(ldx=15), b"ldx"),                        # narrower than nb * D
    (dict(B=1 << 23, ldx=1 << 7), b"4 GiB"),       # B * ldx spans >= 4 GiB
])
def test_seed_rejects_bad_arguments(kw, text):
    rc, msg = _seed(**kw)
    assert rc == 1, (rc, msg)
    assert msg and text in msg, msg


def test_centroids_rejects_bad_arguments():
    h = L.lib()

    def call(parts=P, nparts=1, count=100, nb=4, M=16, W=4, cent=P, ldw=4, bstride=64, update=1):
        rc = h.vqgnn_kmeans_centroids(parts, nparts, count, nb, M, W, cent, ldw, bstride, update,
                                      None, None, None)
        return rc, h.vqgnn_last_error()

    for kw, text in ((dict(parts=None), b"null"), (dict(cent=None), b"null"),
                     (dict(W=9, ldw=9, bstride=144), b"W=9"), (dict(ldw=3), b"layout"),
                     (dict(bstride=63), b"layout"), (dict(count=0), b"shape"),
                     (dict(nparts=0), b"shape")):
        rc, msg = call(**kw)
        assert rc == 1 and msg and text in msg, (kw, rc, msg)


def test_workspace_query_is_monotone():
    h = L.lib()
    ws = h.vqgnn_kmeans_workspace
    assert ws(0, 4, 16, 4) == 0 and ws(100, 4, 16, 9) == 0
    # Z [nb][B][W] + mind [nb][B] floats at the least
    assert ws(84670, 32, 256, 4) >= 84670 * 32 * 5 * 4
    prev = 0
    for B in (1, 63, 64, 1000, 1024, 1025, 4097, 84670, 1 << 23):
        cur = ws(B, 4, 1, 4)
        assert cur > 0 and cur >= prev, (B, cur, prev)
        prev = cur
    prev = 0
    for M in (1, 16, 256, 4096, 32767):
        cur = ws(40000, 4, M, 4)
        assert cur > 0 and cur >= prev, (M, cur, prev)
        prev = cur


def test_wrappers_refuse_cpu_tensors():
    X = torch.zeros(10, 8)
    coef = torch.zeros(6, 8)
    with pytest.raises(RuntimeError, match="only on the GPU"):
        kernels.kmeans_seed(X, coef, 4, 4)
    with pytest.raises(RuntimeError, match="only on the GPU"):
        kernels.kmeans_centroids(torch.zeros(1, 2, 4, 5, dtype=torch.int64), torch.zeros(2, 4, 4),
                                 10)
    bank = VQBank(2, 4, 4)
    with pytest.raises(RuntimeError, match="only on the GPU"):
        bank.kmeans_fit(X, 0, 2, 1, 0)
    bank.comm = object()
    with pytest.raises(NotImplementedError):
        bank.kmeans_fit(X, 0, 2, 1, 0)


def test_layer_keyword_defaults_off():
    from vq_gnn_amd.models import LowRankGNN
    m = LowRankGNN(8, 8, 3, 2, 0.0, 4, 4, 20, no_second_fc=True, grad_scale=[1, 1])
    assert all(c.device_kmeans_init is False and c.kmeans_seed == 0 for c in m.convs)
    m = LowRankGNN(8, 8, 3, 2, 0.0, 4, 4, 20, no_second_fc=True, grad_scale=[1, 1],
                   kmeans_iter=7, device_kmeans_init=True, kmeans_seed=5)
    assert all(c.device_kmeans_init and c.kmeans_seed == 5 and c.kmeans_iter == 7
               for c in m.convs)


def test_restatement_fma_is_a_single_rounding():
    """kmeans_ref.fma32 against exact rational arithmetic, including products
    whose fp64 sum would round twice."""
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, 4000)).astype(np.float32)
    # a b = 1 - 2^-46: the fp64 sum lands exactly halfway between two fp32
    # values and ties-to-even would then round the wrong way
    a[:4], b[:4] = np.float32(1 + 2.0 ** -23), np.float32(1 - 2.0 ** -23)
    c[:4] = np.float32([2.0 ** 24 + 2, -(2.0 ** 24 + 2), 2.0 ** 25 + 4, -(2.0 ** 25 + 4)])
    got = kmeans_ref.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        # Fraction -> float is correctly rounded; fp32 needs its own rounding
        lo = np.float32(float(exact))
        cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))),
                 float(np.nextafter(lo, np.float32(-np.inf)))}
        best = min(cands, key=lambda v: (abs(Fraction(v) - exact),
                                         int(np.float32(v).view(np.uint32)) & 1))
        assert float(got[i]) == best, (i, a[i], b[i], c[i], got[i], best)


def test_restatement_seeding_rules():
    """The draw, the weight and the T = 0 rule of the restatement itself."""
    assert kmeans_ref.draw(3, 1, 2) == kmeans_ref.walk_mix(
        (kmeans_ref.walk_mix(3 ^ kmeans_ref.walk_mix(1)) + 2) & ((1 << 64) - 1))
    q = kmeans_ref.weights(np.float32([0.0, 2.0 ** -21, 3 * 2.0 ** -21, 1.0, 2.0 ** 20, np.inf]))
    assert q.tolist() == [0, 0, 2, 1 << 20, 1 << 40, 1 << 40]      # ties to even, capped
    z = np.repeat(np.arange(5, dtype=np.float32)[:, None], 2, 1)      # 5 distinct rows, exact
    z = np.concatenate([z, z, z])
    rows, cent, zero_steps = kmeans_ref.seed_branch(z, 8, 11, 0)
    assert zero_steps == 3 and len({tuple(c) for c in cent}) == 5
    assert rows[0] == kmeans_ref.draw(11, 0, 0) % 15
    assert [int(r) for r in rows[5:]] == [kmeans_ref.draw(11, 0, s) % 15 for s in (5, 6, 7)]
