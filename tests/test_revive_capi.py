"""C-ABI of the dead-codeword revival (include/vqgnn.h §13): the entries exist
and are bound, reject bad arguments before any launch, the host layer raises
before touching the device, and VQBank.health on a CPU bank.  No GPU here:
every pointer below is a dummy address that validation never dereferences."""
import numpy as np
import pytest
import torch

import vq_gnn_amd._lib as L
from vq_gnn_amd import kernels
from vq_gnn_amd.vq import VQBank

import revive_ref

P = 4096      # dummy non-null device address


def _revive(X=P, ldx=16, B=100, nb=4, D=4, M=16, coef=P, labels=P, threshold=1e-2, R=4,
            init_count=1.0, seed=0, cs=P, cs_bstride=None, ema_w=P, emb=P, emb_out=P, ldw=8,
            bstride=None, rm=P, rv=P, codes=None, ldc=0, bidx=None, n_slots=P, slots=P, rows=P,
            ws=P):
    h = L.lib()
    cs_bstride = M if cs_bstride is None else cs_bstride
    bstride = M * ldw if bstride is None else bstride
    rc = h.vqgnn_vq_revive(X, ldx, B, nb, D, M, coef, labels, threshold, R, init_count, seed, cs,
                           cs_bstride, ema_w, emb, emb_out, ldw, bstride, rm, rv, codes, ldc, bidx,
                           n_slots, slots, rows, ws, None)
    return rc, h.vqgnn_last_error()


def test_entries_exist_and_are_bound():
    h = L.lib()
    for name in ("vqgnn_vq_revive_workspace", "vqgnn_vq_revive"):
        assert name in L.SIGNATURES
        fn = getattr(h, name)
        assert fn.argtypes == L.SIGNATURES[name][1]
    assert callable(kernels.vq_revive)
    assert callable(VQBank.revive) and callable(VQBank.health)


@pytest.mark.parametrize("kw,text", [
    (dict(X=None), b"null"),
    (dict(coef=None), b"null"),
    (dict(labels=None), b"null"),
    (dict(cs=None), b"null"),
    (dict(ema_w=None), b"null"),
    (dict(emb=None), b"null"),
    (dict(emb_out=None), b"null"),
    (dict(rm=None), b"null"),
    (dict(rv=None), b"null"),
    (dict(n_slots=None), b"null"),
    (dict(slots=None), b"null"),
    (dict(rows=None), b"null"),
    (dict(ws=None), b"null"),
    (dict(M=101, R=4), b"M=101"),                      # M > B
    (dict(D=9, ldx=36, ldw=18), b"D=9"),               # D > 8
    (dict(B=(1 << 23) + 1, ldx=16), b"2^23"),
    (dict(B=40000, M=32768), b"int16"),
    (dict(R=0), b"max_revive=0"),
    (dict(R=17), b"max_revive=17"),                    # R > M
    (dict(ldx=15), b"ldx"),
    (dict(B=1 << 23, ldx=1 << 7), b"4 GiB"),
    (dict(ldw=6), b"layout"),                          # neither D nor >= 2D
    (dict(bstride=127), b"layout"),
    (dict(cs_bstride=15), b"layout"),
    (dict(init_count=1e-3), b"init_count"),            # the revived would stay dead
    (dict(codes=P, ldc=4), b"batch_idx"),
    (dict(codes=P, bidx=P, ldc=3), b"ldc"),
])
def test_revive_rejects_bad_arguments(kw, text):
    rc, msg = _revive(**kw)
    assert rc == 1, (rc, msg)
    assert msg and text in msg, msg


def test_workspace_query():
    ws = L.lib().vqgnn_vq_revive_workspace
    for bad in ((0, 4, 4, 16, 4), (100, 0, 4, 16, 4), (100, 4, 0, 16, 4), (100, 4, 9, 16, 4),
                (100, 4, 4, 0, 1), (100, 4, 4, 101, 4), ((1 << 23) + 1, 4, 4, 16, 4),
                (40000, 4, 4, 32768, 4), (100, 4, 4, 16, 0), (100, 4, 4, 16, 17)):
        assert ws(*bad) == 0, bad
    # Z [nb][B][D] + mind [nb][B] floats at the least
    assert ws(84670, 32, 4, 256, 32) >= 84670 * 32 * 5 * 4
    assert ws(100, 4, 4, 16, 16) > 0 and ws(1 << 23, 1, 1, 1, 1) > 0


def test_bank_revive_raises_before_the_device():
    X = torch.zeros(10, 8)
    bank = VQBank(2, 4, 4)
    with pytest.raises(ValueError, match="init_count"):
        bank.revive(X, 0, 2, 1e-2, 0, 2, init_count=1e-3)
    for R in (0, 5):
        with pytest.raises(ValueError, match="max_revive"):
            bank.revive(X, 0, 2, 1e-2, 0, R)
    with pytest.raises(ValueError, match="codewords from"):
        bank.revive(X[:3], 0, 2, 1e-2, 0, 2)                      # M > B
    with pytest.raises(RuntimeError, match="only on the GPU"):
        bank.revive(X, 0, 2, 1e-2, 0, 2)
    bank.comm = object()
    with pytest.raises(NotImplementedError):
        bank.revive(X, 0, 2, 1e-2, 0, 2)


def test_wrapper_refuses_cpu_tensors():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="only on the GPU"):
        kernels.vq_revive(z(10, 8), z(6, 8), z(2, 10, dtype=torch.int64), 4, 1e-2, 2, 1.0, 0,
                          z(2, 4), z(2, 4, 8), z(2, 4, 8), z(2, 4, 8), z(2, 4), z(2, 4))


def test_health_on_a_cpu_bank():
    nb, M = 4, 37
    bank = VQBank(nb, M, 4)
    cs = torch.zeros(nb, M)
    cs[0] = 2.5                                     # uniform: perplexity M, nothing dead
    cs[1, 11] = 3.0                                 # one nonzero entry: perplexity 1
    cs[2] = 1.0
    cs[2, [0, 5, 36]] = torch.tensor([0.0, 9e-3, 1e-2])   # 1e-2 is not < 1e-2
    cs[3, :10] = 1.0                                # ten equal entries: perplexity 10
    bank.cs.copy_(cs)
    n_dead, perp = bank.health(1e-2)
    assert n_dead.dtype == torch.int32 and perp.dtype == torch.float32
    assert n_dead.tolist() == [0, M - 1, 2, M - 10]
    np.testing.assert_allclose(perp[[0, 1, 3]].numpy(), [M, 1.0, 10.0], rtol=1e-6)
    assert 1.0 < float(perp[2]) < M


def test_layer_keywords_default_off():
    from vq_gnn_amd.models import LowRankGNN
    m = LowRankGNN(8, 8, 3, 2, 0.0, 16, 4, 20, no_second_fc=True, grad_scale=[1, 1])
    for c in m.convs:
        assert c.revive_dead_every == 0 and c.revive_threshold == 1e-2
        assert c.revive_max == 2 and c.revive_init_count == 1.0 and c.revive_result is None
        n_dead, perp = c.codebook_health()
        assert n_dead.shape == (c.num_branch,) and perp.shape == (c.num_branch,)
    m = LowRankGNN(8, 8, 3, 2, 0.0, 4, 4, 20, no_second_fc=True, grad_scale=[1, 1],
                   revive_dead_every=3, revive_threshold=0.5, revive_max=4, revive_init_count=2.0)
    assert all((c.revive_dead_every, c.revive_threshold, c.revive_max, c.revive_init_count) ==
               (3, 0.5, 4, 2.0) for c in m.convs)
    assert LowRankGNN(8, 8, 3, 2, 0.0, 4, 4, 20, no_second_fc=True,
                      grad_scale=[1, 1]).convs[0].revive_max == 1      # max(1, 4 // 8)


def test_restatement_rules():
    """The slot rule, the initial mind, the T = 0 rule and the layer seed of
    the restatement itself."""
    F32 = np.float32
    assert revive_ref.layer_seed(5, 3) == revive_ref.walk_mix(5 ^ revive_ref.walk_mix(3))
    # 6 points on a line, 4 codewords: 0 and 3 live on points 0 and 5, 1 (NaN)
    # and 2 (dead); labels: nearest live codeword, one out of range
    z = np.arange(6, dtype=F32)[:, None] * np.ones((1, 2), F32)
    emb = np.zeros((4, 4), F32)
    emb[3, :2] = 5.0
    emb[:, 2:] = [[1, 2], [3, 4], [5, 6], [7, 8]]
    cs = np.array([1.0, np.nan, 0.0, 1.0], F32)
    ema_w, emb_out = emb.copy(), emb.copy()
    labels = np.array([0, 0, 0, 3, 7, 3], np.int64)
    mind = revive_ref.initial_mind(z, emb[:, :2], labels)
    assert mind.tolist() == [0.0, 2.0, 8.0, 8.0, 0.0, 0.0]
    rm, rv = np.array([1.0, -1.0], F32), np.array([4.0, 9.0], F32) - F32(1e-5)
    n, slots, rows, zero = revive_ref.revive_branch(z, 0, cs, emb, ema_w, emb_out, labels, rm, rv,
                                                    1e-2, 3, 2.0, 11)
    assert (n, slots.tolist(), zero) == (1, [2, -1, -1], 0)       # the NaN is not dead
    i = int(rows[0])
    assert i in (1, 2, 3) and rows[1:].tolist() == [-1, -1]
    q = revive_ref.weights(mind)
    t = revive_ref.draw(11, 0, 0) % int(q.sum())
    assert i == int(np.nonzero(np.cumsum(q) > t)[0][0])
    assert emb[2].tolist() == [i, i, 5, 6] and cs[2] == 2.0
    assert ema_w[2].tolist() == [2 * i, 2 * i, 10, 12]
    sd = np.sqrt((rv + F32(1e-5)).astype(F32))
    assert emb_out[2].tolist() == [float(F32(i) * sd[0] + rm[0]), float(F32(i) * sd[1] + rm[1]),
                                   5, 6]
    # every row a codeword's copy: T = 0, the row is r mod B
    row, zero = revive_ref.pick(np.zeros(6, F32), 12345)
    assert (row, zero) == (12345 % 6, True)
