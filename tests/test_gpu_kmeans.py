"""Device k-means++ codebook initialisation (include/vqgnn.h §12) against the
numpy restatement tests/kmeans_ref.py: seeding bit for bit, the Lloyd steps,
the empty-cluster rule, determinism, untouched bank state and the layer
keyword ``device_kmeans_init``."""
import numpy as np
import pytest
import torch

import kmeans_ref
from helpers import tie_aware_mismatch
from oracle import vq_ref
from vq_gnn_amd import graph, kernels
from vq_gnn_amd.kernels import BN_TRAIN
from vq_gnn_amd.models import LowRankGNNLayer
from vq_gnn_amd.vq import VQBank

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PART = 1024      # rows per part of the seeding kernels (csrc/kmeans_kernels.hip, kKmPart)


def _coef(nb, D, rng, identity=False):
    """A coefficient table [6, nb*D] in vqgnn_vq_assign's layout (alpha_f,
    beta_f, alpha_g, beta_g, shift_f, shift_g)."""
    F = nb * D
    coef = np.zeros((6, F), np.float32)
    if identity:
        coef[0] = 1.0
    else:
        coef[0] = rng.uniform(0.5, 2.0, F)
        coef[1] = rng.standard_normal(F) * 0.1
        coef[4] = rng.standard_normal(F) * 0.3
    return coef


def _on_device(X, strided):
    """X [B, F] on the device: contiguous, or a column slice of a wider matrix
    (any ldx the assign accepts)."""
    t = torch.from_numpy(X)
    if not strided:
        return t.to(DEV).contiguous()
    wide = torch.zeros(X.shape[0], X.shape[1] + 12, dtype=torch.float32, device=DEV)
    wide[:, 4:4 + X.shape[1]] = t.to(DEV)
    return wide[:, 4:4 + X.shape[1]]


def _seed_case(X, coef, D, M, seed, strided):
    nb = X.shape[1] // D
    cent, rows = kernels.kmeans_seed(_on_device(X, strided), torch.from_numpy(coef).to(DEV), D, M,
                                     seed)
    torch.cuda.synchronize()
    cent, rows = cent.cpu().numpy(), rows.cpu().numpy()
    zero_steps = 0
    for b in range(nb):
        z = kmeans_ref.normalise(X, coef, b, D)
        r_rows, r_cent, zs = kmeans_ref.seed_branch(z, M, seed, b)
        zero_steps += zs
        assert rows[b].tolist() == r_rows.tolist(), f"branch {b}: seed rows differ"
        assert cent[b].tobytes() == r_cent.tobytes(), f"branch {b}: centroids differ"
    return rows, zero_steps


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("B,nb,D,M", [(300, 3, 4, 37), (1000, 2, 2, 64)])
def test_seeding_matches_restatement(B, nb, D, M, strided):
    rng = np.random.default_rng(B)
    X = rng.standard_normal((B, nb * D)).astype(np.float32)
    _seed_case(X, _coef(nb, D, rng), D, M, seed=B + 7, strided=strided)


@pytest.mark.parametrize("strided", [False, True])
def test_seeding_every_distinct_row_a_seed(strided):
    """B = 64, M = 16: 16 distinct rows, B / M copies of each.  Every distinct
    row becomes a seed; the copies of a seed have d = 0 up to rounding and the
    seed itself exactly 0 (the zeroed mind)."""
    rng = np.random.default_rng(64)
    nb, D, M = 2, 4, 16
    base = rng.standard_normal((16, nb * D)).astype(np.float32)
    X = base[rng.permutation(np.repeat(np.arange(16), 4))]
    rows, _ = _seed_case(X, _coef(nb, D, rng), D, M, seed=3, strided=strided)
    for b in range(nb):
        picked = {X[r, b * D:(b + 1) * D].tobytes() for r in rows[b]}
        assert len(picked) == 16


@pytest.mark.parametrize("strided", [False, True])
def test_seeding_with_fewer_distinct_rows_than_seeds(strided):
    """B = 48, M = 16, only 10 distinct rows (small integers: every distance
    is exact): after 10 steps T = 0 and the draw falls back to r mod B."""
    rng = np.random.default_rng(48)
    nb, D, M = 2, 4, 16
    base = np.unique(rng.integers(-3, 4, (40, nb * D)), axis=0)[:10].astype(np.float32)
    assert base.shape[0] == 10
    for b in range(nb):      # distinct inside every branch, too
        assert np.unique(base[:, b * D:(b + 1) * D], axis=0).shape[0] == 10
    X = base[rng.permutation(np.resize(np.arange(10), 48))]
    _, zero_steps = _seed_case(X, _coef(nb, D, rng, identity=True), D, M, seed=5, strided=strided)
    assert zero_steps == nb * (M - 10)       # the restatement took the T = 0 branch


@pytest.mark.parametrize("strided", [False, True])
def test_seeding_spans_row_parts(strided):
    """B reaches four row parts with a ragged last one; seeds must come from
    every part for the part scan to matter."""
    rng = np.random.default_rng(7)
    nb, D, M = 2, 3, 8
    B = 3 * PART + 37
    X = rng.standard_normal((B, nb * D)).astype(np.float32)
    rows, _ = _seed_case(X, _coef(nb, D, rng), D, M, seed=1, strided=strided)
    assert len({int(r) // PART for r in rows.ravel()}) >= 3


# --------------------------------------------------------------------------- #
def _bank_coef(bank, Xd, nbr):
    """The coefficients a training-mode feature_update computes for Xd, on
    throwaway running statistics."""
    ax, _ = bank._arith(Xd, None)
    coef, _, _ = kernels.bn_stats_finalize(Xd, None, nbr * bank.D, BN_TRAIN, 0.1, 1e-5, 0.0, 0.0,
                                           0.0, bank.rm_f.clone(), bank.rv_f.clone(), D=bank.D,
                                           arith_x=ax, ref_threads=bank._threads())
    return coef.cpu().numpy()


@pytest.fixture(scope="module")
def fit_case():
    """B = 2,000, nb = 4, D = 4, M = 64, iters = 3: the restatement's fit of
    every branch, computed once."""
    rng = np.random.default_rng(2000)
    B, nb, D, M, iters, seed = 2000, 4, 4, 64, 3, 17
    X = (rng.standard_normal((B, nb * D)) * rng.uniform(0.5, 3.0, nb * D) +
         rng.standard_normal(nb * D)).astype(np.float32)
    bank = VQBank(nb, M, D).to(DEV)
    Xd = torch.from_numpy(X).to(DEV)
    coef = _bank_coef(bank, Xd, nb)
    Z = [kmeans_ref.normalise(X, coef, b, D) for b in range(nb)]
    ref = [kmeans_ref.fit_branch(Z[b], M, iters, seed, b) for b in range(nb)]
    return dict(B=B, nb=nb, D=D, M=M, iters=iters, seed=seed, X=X, Xd=Xd, Z=Z, ref=ref)


@pytest.mark.parametrize("iters", [0, 1, 2, 3])
def test_fit_matches_restatement(fit_case, iters):
    """A fit of ``iters`` Lloyd steps ends on the restatement's centroids of
    that iteration (bit for bit), with the labels and counts of the assign
    against them; the labels are oracle/vq_ref.py's argmin."""
    c = fit_case
    bank = VQBank(c["nb"], c["M"], c["D"]).to(DEV)
    cent, counts, labels, rows = bank.kmeans_fit(c["Xd"], 0, c["nb"], iters, c["seed"])
    torch.cuda.synchronize()
    cent, counts, labels, rows = (t.cpu().numpy() for t in (cent, counts, labels, rows))
    empty = 0
    for b in range(c["nb"]):
        r = c["ref"][b]
        assert rows[b].tolist() == r["seed_rows"].tolist()
        assert cent[b].tobytes() == r["centroids"][iters].tobytes(), f"branch {b} centroids"
        assert np.array_equal(labels[b], r["labels"][iters]), f"branch {b} labels"
        assert np.array_equal(counts[b], r["counts"][iters]), f"branch {b} counts"
        assert counts[b].sum() == c["B"]
        empty += int((r["counts"][iters] == 0).sum())
        # oracle/vq_ref.py's distances and argmin on the same points and
        # centroids; a row may differ only where the oracle's own two
        # distances tie to 1e-5 (its sgemm's rounding, helpers.py)
        d = vq_ref.distances(torch.from_numpy(c["Z"][b]), torch.from_numpy(cent[b]))
        _, unexplained = tie_aware_mismatch(torch.argmin(d, dim=1), labels[b], d)
        assert unexplained == 0
    assert int(bank.kmeans_n_empty.item()) == empty


def test_empty_cluster_keeps_its_centroid():
    """Duplicate seeds (10 distinct rows, M = 16): the later copy of a
    centroid loses every tie to the first index, so its cluster is empty; it
    keeps its centroid, has count 0, and n_empty reports it."""
    rng = np.random.default_rng(48)
    nb, D, M, B = 2, 4, 16, 48
    base = np.unique(rng.integers(-3, 4, (40, nb * D)), axis=0)[:10].astype(np.float32)
    X = base[rng.permutation(np.resize(np.arange(10), B))]
    coef = _coef(nb, D, rng, identity=True)
    Xd, cd = torch.from_numpy(X).to(DEV), torch.from_numpy(coef).to(DEV)
    cent, _ = kernels.kmeans_seed(Xd, cd, D, M, 5)
    before = cent.clone()
    labels = torch.empty(nb, B, dtype=torch.int64, device=DEV)
    stats = kernels.vq_assign(Xd, None, cd, 1.0, cent, D, D, idx_out=labels, want_stats=True,
                              stat_count=B)
    counts, n_empty = kernels.kmeans_centroids(stats, cent, B, update=True)
    torch.cuda.synchronize()
    assert int(stats.abs().sum()) == 0                      # the slab is cleared
    counts_h, cent_h, before_h = counts.cpu().numpy(), cent.cpu().numpy(), before.cpu().numpy()
    shift = kmeans_ref.stat_shift(B)
    for b in range(nb):
        z = kmeans_ref.normalise(X, coef, b, D)
        lab = kmeans_ref.assign(z, before_h[b])
        r_counts, r_cent = kmeans_ref.lloyd_step(z, before_h[b], lab, shift)
        assert np.array_equal(labels[b].cpu().numpy(), lab)
        assert np.array_equal(counts_h[b], r_counts)
        assert cent_h[b].tobytes() == r_cent.tobytes()
        gone = counts_h[b] == 0
        assert gone.sum() == M - 10
        assert cent_h[b][gone].tobytes() == before_h[b][gone].tobytes()
    assert int(n_empty.item()) == nb * (M - 10)


def test_fit_is_deterministic_per_seed(fit_case):
    c = fit_case
    bank = VQBank(c["nb"], c["M"], c["D"]).to(DEV)
    a = bank.kmeans_fit(c["Xd"], 0, c["nb"], 2, 5)
    b = bank.kmeans_fit(c["Xd"], 0, c["nb"], 2, 5)
    o = bank.kmeans_fit(c["Xd"], 0, c["nb"], 2, 6)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[3], o[3])


def test_fit_leaves_the_bank_untouched(fit_case):
    c = fit_case
    nb = c["nb"]
    bank = VQBank(nb, c["M"], c["D"]).to(DEV)
    for b in range(nb):
        bank.init_branch(b)
    bank.rm_f.normal_()
    bank.rv_f.uniform_(0.5, 2.0)
    bank.nbt_f.fill_(3)
    N = 2500
    codes = torch.full((N, nb), -1, dtype=torch.int16, device=DEV)
    bidx = torch.randperm(N, device=DEV)[:c["B"]]
    state = {k: v.clone() for k, v in bank.named_buffers()}
    _, _, labels, _ = bank.kmeans_fit(c["Xd"], 0, nb, 1, c["seed"], codes=codes, batch_idx=bidx)
    torch.cuda.synchronize()
    for k, v in bank.named_buffers():
        assert torch.equal(v, state[k]), f"kmeans_fit changed {k}"
    assert int(bank.stats_f.abs().sum()) == 0 and int(bank.stats_u.abs().sum()) == 0
    assert not any(bank._dirty[c["D"]])
    # the labels went through codes / batch_idx like any assign's
    assert torch.equal(codes[bidx].long(), labels.t())
    mask = torch.ones(N, dtype=torch.bool, device=DEV)
    mask[bidx] = False
    assert bool((codes[mask] == -1).all())


# --------------------------------------------------------------------------- #
def _blobs(rng, B, F, k, spread):
    centres = rng.standard_normal((k, F)).astype(np.float32) * 2.0
    which = rng.integers(0, k, B)
    return (centres[which] + spread * rng.standard_normal((B, F))).astype(np.float32), which


def _layer(F_in, F_out, M, N, kmeans_iter, **kw):
    # warm_up_flag=False: the first feature_update raises 'Bad Init!' on an
    # empty cluster (vq.py:188-189)
    return LowRankGNNLayer(F_in, F_out, 0.0, M, 4, N, 0, 'vq', False, True, kmeans_iter, True,
                           True, False, 0, False, False, 0.5, [1, 1], True, False, False, 0.1,
                           'GCN', False, **kw)


def test_layer_device_kmeans_init_cures_bad_init():
    """Rows from 8 tight blobs, B = 2,000, F = 16, D = 4, M = 64, no warm-up.
    The blob spread is 0.01 of the blob distance: after BatchNorm a branch's
    rows sit in 8 clumps, so of 64 N(0, 1) codewords at most a few per clump
    are nearest to anything and the rest own no row -- the default layer
    raises 'Bad Init!' (asserted first: today's behaviour).  With
    device_kmeans_init=True the same layer completes."""
    rng = np.random.default_rng(8)
    B, F, D, M, iters, seed = 2000, 16, 4, 64, 3, 9
    x_h, _ = _blobs(rng, B, F, 8, 0.01)
    g = graph.synthetic_graph(2500, 5, 9000, seed=3)
    rp, cl, vl = graph.norm_adj(g, "GCN")
    b = graph.k_hop_batch(rp, cl, vl, g.N, np.arange(B))
    assert b.B == B
    batch_A = graph.batch_to_device(b, DEV)
    x = torch.from_numpy(x_h).to(DEV)

    torch.manual_seed(0)
    default = _layer(F, 8, M, g.N, iters).to(DEV).train()
    with pytest.raises(ValueError, match="Bad Init!"):
        default(x, batch_A, 1.0, False)

    torch.manual_seed(0)
    layer = _layer(F, 8, M, g.N, iters, device_kmeans_init=True, kmeans_seed=seed).to(DEV).train()
    # setup check on the restatement alone: this data and seed leave no
    # cluster empty, so a zero below would be the device's doing
    coef = _bank_coef(layer._bank, x, F // D)
    for br in range(F // D):
        r = kmeans_ref.fit_branch(kmeans_ref.normalise(x_h, coef, br, D), M, iters, seed, br)
        assert (r["counts"][iters] > 0).all(), "setup: the restatement left a cluster empty"
    out = layer(x, batch_A, 1.0, False)[0]
    assert out.shape == (B, 8) and bool(torch.isfinite(out).all())
    cent, counts, labels, _ = layer.kmeans_result
    assert torch.equal(layer._codes[batch_A[0]].long(), labels.t())
    for br, blk in enumerate(layer.gnn_block):
        assert torch.equal(blk.c_indices[batch_A[0]].long(), labels[br])
        assert int((blk.vq._ema_cluster_size == 0).sum()) == 0
    assert int(layer._bank.nbt_f.min()) == 1          # the init path ran once, after the fit
    fitted = layer.kmeans_result
    layer(x, batch_A, 1.0, False)                     # a second training forward: no raise
    assert layer.kmeans_result is fitted              # and no second fit


def test_planted_partition_is_recovered():
    """16 well-separated blobs, M = 16: the restatement alone must recover the
    partition for this seed (a setup failure otherwise), and the device
    labels must equal the restatement's."""
    rng = np.random.default_rng(16)
    B, nb, D, M, iters, seed = 800, 2, 4, 16, 2, 4
    X, which = _blobs(rng, B, nb * D, 16, 0.01)
    bank = VQBank(nb, M, D).to(DEV)
    Xd = torch.from_numpy(X).to(DEV)
    coef = _bank_coef(bank, Xd, nb)
    refs = []
    for b in range(nb):
        r = kmeans_ref.fit_branch(kmeans_ref.normalise(X, coef, b, D), M, iters, seed, b)
        lab = r["labels"][iters]
        pairs = set(zip(which.tolist(), lab.tolist()))
        assert len(pairs) == 16 and len({p[1] for p in pairs}) == 16, \
            "setup: the restatement did not recover the planted partition for this seed"
        refs.append(lab)
    _, counts, labels, _ = bank.kmeans_fit(Xd, 0, nb, iters, seed)
    torch.cuda.synchronize()
    for b in range(nb):
        assert np.array_equal(labels[b].cpu().numpy(), refs[b])
        assert np.array_equal(counts[b].cpu().numpy(), np.bincount(refs[b], minlength=M))
