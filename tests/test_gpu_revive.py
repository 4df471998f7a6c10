"""Dead-codeword revival on the device (include/vqgnn.h §13) against the numpy
restatement tests/revive_ref.py: bit for bit, nothing else written, the cap
and the order of the slots, the T = 0 rule, determinism, the job it is for,
the code scatter, bad labels, and the layer options."""
import functools

import numpy as np
import pytest
import torch

import kmeans_ref
import revive_ref
from vq_gnn_amd import graph, kernels
from vq_gnn_amd.kernels import BN_TRAIN
from vq_gnn_amd.models import LowRankGNNLayer
from vq_gnn_amd.vq import VQBank

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PART = 1024      # rows per part of the seeding kernels (csrc/kmeans_kernels.hip, kKmPart)
THR = 1e-2
# (B, nb, D, M): the k-means tests' shapes; the last one's prefix sum crosses row parts
SHAPES = [(300, 3, 4, 37), (1000, 2, 2, 64), (3 * PART + 37, 2, 3, 8)]
# dead codewords per branch: one branch with none, one over R = 1 and 5
DEAD = {37: (0, 9, 37), 64: (0, 20), 8: (0, 7)}
STATE = ("cs", "emb", "ema_w", "emb_out")


def _coef(nb, D, rng, identity=False):
    """A coefficient table [6, nb*D] in vqgnn_vq_assign's layout."""
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
    t = torch.from_numpy(X)
    if not strided:
        return t.to(DEV).contiguous()
    wide = torch.zeros(X.shape[0], X.shape[1] + 12, dtype=torch.float32, device=DEV)
    wide[:, 4:4 + X.shape[1]] = t.to(DEV)
    return wide[:, 4:4 + X.shape[1]]


def _state(rng, nb, D, M, dead):
    """A random bank state as numpy arrays, ``dead[b]`` codewords of branch b
    below the threshold (zeros and small values, at random positions)."""
    st = dict(emb=rng.standard_normal((nb, M, 2 * D)), ema_w=rng.standard_normal((nb, M, 2 * D)),
              emb_out=rng.standard_normal((nb, M, 2 * D)), cs=rng.uniform(0.5, 5.0, (nb, M)),
              rm_f=rng.standard_normal((nb, D)), rv_f=rng.uniform(0.5, 2.0, (nb, D)),
              rm_g=rng.standard_normal((nb, D)), rv_g=rng.uniform(0.5, 2.0, (nb, D)))
    st = {k: v.astype(np.float32) for k, v in st.items()}
    for b, n in enumerate(dead):
        where = rng.permutation(M)[:n]
        st["cs"][b, where] = rng.choice(np.float32([0.0, 1e-3, 9.9e-3]), n)
    return st


def _bank(st, nb, D, M):
    bank = VQBank(nb, M, D).to(DEV)
    for k, v in st.items():
        getattr(bank, k).copy_(torch.from_numpy(v))
    bank.nbt_f.fill_(3)
    bank.nbt_g.fill_(2)
    return bank


def _labels(X, coef, D, emb):
    return np.stack([kmeans_ref.assign(kmeans_ref.normalise(X, coef, b, D), emb[b, :, :D])
                     for b in range(emb.shape[0])])


def _call(bank, Xd, coef, labels, R, seed, init_count=1.0, codes=None, batch_idx=None):
    """The C-ABI entry on the bank's tensors with given coefficients / labels."""
    out = kernels.vq_revive(Xd, torch.from_numpy(coef).to(DEV), torch.from_numpy(labels).to(DEV),
                            bank.D, THR, R, init_count, seed, bank.cs, bank.ema_w, bank.emb,
                            bank.emb_out, bank.rm_f, bank.rv_f, codes=codes, batch_idx=batch_idx)
    torch.cuda.synchronize()
    return out


def _same_bits(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


@functools.lru_cache(maxsize=None)
def _case(shape, R):
    """Inputs, bank state and the restatement's result for one (shape, R),
    computed once and never changed."""
    B, nb, D, M = shape
    rng = np.random.default_rng(B + R)
    X = rng.standard_normal((B, nb * D)).astype(np.float32)
    coef = _coef(nb, D, rng)
    st = _state(rng, nb, D, M, DEAD[M])
    labels = _labels(X, coef, D, st["emb"])
    seed = B + 7
    ref = revive_ref.revive(X, coef, D, st, labels, THR, R, 1.5, seed)
    return dict(X=X, coef=coef, st=st, labels=labels, seed=seed, ref=ref, init_count=1.5)


def _check_against(ref, bank, out):
    n_slots, slots, rows = out
    assert n_slots.cpu().numpy().tolist() == ref["n_slots"].tolist()
    assert torch.equal(slots.cpu(), torch.from_numpy(ref["slots"]))
    assert torch.equal(rows.cpu(), torch.from_numpy(ref["rows"]))
    for k in STATE:
        assert _same_bits(getattr(bank, k), ref[k]), f"{k} differs from the restatement"


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("R", [1, 5, "M"])
@pytest.mark.parametrize("shape", SHAPES)
def test_matches_restatement_and_moves_nothing_else(shape, R, strided):
    """Items 1-3: n_slots, slots, rows and the whole of emb, cs, ema_w, emb_out
    equal the restatement bit for bit; everything §13 does not list is
    bit-identical to before, the slabs stay zero, a branch with no dead
    codeword is untouched; with n_dead > R exactly the R lowest dead m are
    revived."""
    B, nb, D, M = shape
    R = M if R == "M" else R
    c = _case(shape, R)
    bank = _bank(c["st"], nb, D, M)
    before = {k: v.clone() for k, v in bank.named_buffers()}
    out = _call(bank, _on_device(c["X"], strided), c["coef"], c["labels"], R, c["seed"],
                c["init_count"])
    _check_against(c["ref"], bank, out)
    n_slots, slots, rows = (t.cpu().numpy() for t in out)
    # the cap and the order, from the planted state alone
    for b in range(nb):
        dead = np.nonzero(c["st"]["cs"][b] < np.float32(THR))[0]
        assert dead.shape[0] == DEAD[M][b]
        n = min(dead.shape[0], R)
        assert n_slots[b] == n
        assert slots[b].tolist() == dead[:n].tolist() + [-1] * (R - n)
        assert (rows[b, :n] >= 0).all() and (rows[b, :n] < B).all()
        assert (rows[b, n:] == -1).all()
    assert any(DEAD[M][b] > R for b in range(nb)) or R == M
    if B > PART and R == M:            # the draws must come from several row parts
        assert len({int(r) // PART for r in rows.ravel() if r >= 0}) >= 3
    # nothing else moves
    after = dict(bank.named_buffers())
    touched = torch.zeros(nb, M, dtype=torch.bool, device=DEV)
    for b in range(nb):
        touched[b, torch.from_numpy(slots[b, :n_slots[b]]).long().to(DEV)] = True
    keep = ~touched
    assert torch.equal(after["cs"][keep], before["cs"][keep])
    for k in ("emb", "ema_w", "emb_out"):
        assert torch.equal(after[k][keep], before[k][keep]), k
    for k in ("emb", "emb_out"):                      # the gradient halves of the revived
        assert torch.equal(after[k][:, :, D:], before[k][:, :, D:]), k
    assert bool((after["cs"][touched] == c["init_count"]).all())
    for k in before:
        if k not in STATE:
            assert torch.equal(after[k], before[k]), f"revive changed {k}"
    assert int(bank.stats_f.abs().sum()) == 0 and int(bank.stats_u.abs().sum()) == 0
    assert int(bank.bad_flag.item()) == 0
    assert DEAD[M][0] == 0
    for k in STATE:
        assert torch.equal(after[k][0], before[k][0]), f"branch 0 has no dead codeword: {k}"


def test_nan_cluster_size_is_not_dead():
    B, nb, D, M = SHAPES[0]
    c = _case(SHAPES[0], 5)
    st = {k: v.copy() for k, v in c["st"].items()}
    st["cs"][0, 4] = np.nan
    bank = _bank(st, nb, D, M)
    out = _call(bank, _on_device(c["X"], False), c["coef"], c["labels"], 5, c["seed"])
    assert int(out[0][0]) == 0 and bool((out[1][0] == -1).all())
    assert bool(torch.isnan(bank.cs[0, 4]))


@pytest.mark.parametrize("strided", [False, True])
def test_every_row_a_codeword_draws_r_mod_B(strided):
    """Item 4, T = 0: every row is a copy of a live codeword (small integers,
    identity coefficients: every distance is exactly 0), so each step's row
    is r(b, s) mod B."""
    rng = np.random.default_rng(48)
    B, nb, D, M, R, seed = 48, 2, 4, 16, 6, 5
    base = np.unique(rng.integers(-3, 4, (40, nb * D)), axis=0)[:10].astype(np.float32)
    for b in range(nb):
        assert np.unique(base[:, b * D:(b + 1) * D], axis=0).shape[0] == 10
    which = rng.permutation(np.resize(np.arange(10), B))
    X = base[which]
    coef = _coef(nb, D, rng, identity=True)
    st = _state(rng, nb, D, M, (0, 0))
    for b in range(nb):                   # codewords 0..9 = the distinct rows, 10..15 dead
        st["emb"][b, :10, :D] = base[:, b * D:(b + 1) * D]
        st["cs"][b, 10:] = 0.0
    labels = np.stack([which] * nb).astype(np.int64)
    ref = revive_ref.revive(X, coef, D, st, labels, THR, R, 1.0, seed)
    assert ref["zero_steps"] == nb * R                # the restatement took the T = 0 branch
    bank = _bank(st, nb, D, M)
    out = _call(bank, _on_device(X, strided), coef, labels, R, seed)
    _check_against(ref, bank, out)
    want = [[kmeans_ref.draw(seed, b, s) % B for s in range(R)] for b in range(nb)]
    assert out[2].cpu().numpy().tolist() == want


def test_deterministic_per_seed():
    """Item 5: the same state and seed twice give the same result; another
    seed draws other rows (the restatement's rows for the two seeds differ:
    a setup check, so a device that ignored the seed would fail)."""
    shape = SHAPES[0]
    B, nb, D, M = shape
    c = _case(shape, 5)
    Xd = _on_device(c["X"], False)
    runs = []
    for seed in (c["seed"], c["seed"], c["seed"] + 1):
        bank = _bank(c["st"], nb, D, M)
        out = _call(bank, Xd, c["coef"], c["labels"], 5, seed, c["init_count"])
        runs.append((out, {k: getattr(bank, k).clone() for k in STATE}))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert torch.equal(x, y)
    for k in STATE:
        assert _same_bits(runs[0][1][k], runs[1][1][k].cpu().numpy())
    other = revive_ref.revive(c["X"], c["coef"], D, c["st"], c["labels"], THR, 5, c["init_count"],
                              c["seed"] + 1)
    assert not np.array_equal(other["rows"], c["ref"]["rows"]), "setup: the seeds draw alike"
    assert not torch.equal(runs[0][0][2], runs[2][0][2])
    assert torch.equal(runs[2][0][2].cpu(), torch.from_numpy(other["rows"]))


def _bank_coef(bank, Xd, nbr):
    """The coefficients VQBank.revive computes for Xd (training mode, on
    throwaway running statistics)."""
    ax, _ = bank._arith(Xd, None)
    coef, _, _ = kernels.bn_stats_finalize(Xd, None, nbr * bank.D, BN_TRAIN, 0.1, 1e-5, 0.0, 0.0,
                                           0.0, bank.rm_f.clone(), bank.rv_f.clone(), D=bank.D,
                                           arith_x=ax, ref_threads=bank._threads())
    return coef


def _assign(bank, Xd, coef):
    labels = torch.empty(bank.nb, Xd.shape[0], dtype=torch.int64, device=DEV)
    kernels.vq_assign(Xd, None, coef, 1.0, bank.emb, bank.D, bank.D, idx_out=labels)
    return labels


def _planted(rng, B, nb, D, M):
    """Distinct random rows and a bank whose odd codewords sit far from the
    data (feature halves at +50) with cs = 0."""
    X = rng.standard_normal((B, nb * D)).astype(np.float32)
    assert np.unique(X, axis=0).shape[0] == B
    st = _state(rng, nb, D, M, (0,) * nb)
    st["emb"][:, 1::2, :D] = 50.0
    st["cs"][:, 1::2] = 0.0
    return X, st


def test_bank_revive_does_its_job():
    """Items 6 and 7 through VQBank.revive: half the codewords of every branch
    are far away and dead; after revive(R = M) every revived codeword owns at
    least its own row, the mean quantisation error drops, health reports no
    dead codeword, the rows are distinct, and the codes of the revived rows
    (and no other entry) are the revived slots."""
    B, nb, D, M = SHAPES[0]
    rng = np.random.default_rng(6)
    X, st = _planted(rng, B, nb, D, M)
    bank = _bank(st, nb, D, M)
    Xd = torch.from_numpy(X).to(DEV)
    coef = _bank_coef(bank, Xd, nb)
    coef_h = coef.cpu().numpy()
    Z = [kmeans_ref.normalise(X, coef_h, b, D) for b in range(nb)]
    used = [int(torch.unique(row).numel()) for row in _assign(bank, Xd, coef)]
    assert max(used) <= (M + 1) // 2
    err0 = [revive_ref.nearest_mind(Z[b], st["emb"][b, :, :D]).mean() for b in range(nb)]
    n_dead0 = bank.health(THR)[0]
    assert n_dead0.tolist() == [M // 2] * nb

    N = 500
    codes = torch.full((N, nb), -1, dtype=torch.int16, device=DEV)
    bidx = torch.randperm(N, device=DEV)[:B]
    before = {k: v.clone() for k, v in bank.named_buffers()}
    n_slots, slots, rows = bank.revive(Xd, 0, nb, THR, 21, M, codes=codes, batch_idx=bidx)
    torch.cuda.synchronize()
    assert n_slots.tolist() == [M // 2] * nb
    assert bank.health(THR)[0].tolist() == [0] * nb
    for k in before:
        if k not in STATE:
            assert torch.equal(getattr(bank, k), before[k]), f"revive changed {k}"
    assert not any(bank._dirty[D]) and not any(bank._dirty[2 * D])
    # the restatement from the device's own coefficients and the argmin labels
    ref = revive_ref.revive(X, coef_h, D, st, _labels(X, coef_h, D, st["emb"]), THR, M, 1.0, 21,
                            codes=np.full((N, nb), -1, np.int16), batch_idx=bidx.cpu().numpy())
    _check_against(ref, bank, (n_slots, slots, rows))
    assert torch.equal(codes.cpu(), torch.from_numpy(ref["codes"]))

    counts = [torch.bincount(row, minlength=M) for row in _assign(bank, Xd, coef)]
    emb = bank.emb.cpu().numpy()
    exp_codes = torch.full((N, nb), -1, dtype=torch.int16)
    for b in range(nb):
        n = int(n_slots[b])
        sl, rw = slots[b, :n].long(), rows[b, :n].long()
        assert sl.tolist() == list(range(1, M, 2))
        assert int(torch.unique(rw).numel()) == n, "rows drawn twice"
        assert bool((counts[b][sl] >= 1).all())
        assert revive_ref.nearest_mind(Z[b], emb[b, :, :D]).mean() < err0[b]
        exp_codes[bidx[rw].cpu(), b] = sl.cpu().to(torch.int16)
    assert torch.equal(codes.cpu(), exp_codes)            # item 7: those entries and no other


def test_bad_labels_are_never_drawn():
    """Item 8: labels outside [0, M) give mind = 0: such rows carry no weight,
    the run ends clean and equals the restatement."""
    shape = SHAPES[0]
    B, nb, D, M = shape
    c = _case(shape, 5)
    labels = c["labels"].copy()
    bad = np.arange(0, B, 3)
    labels[:, bad] = np.resize(np.int64([-1, M, 1 << 40, -(1 << 40), M + 7]), bad.shape[0])
    ref = revive_ref.revive(c["X"], c["coef"], D, c["st"], labels, THR, 5, 1.0, c["seed"])
    assert ref["zero_steps"] == 0
    bank = _bank(c["st"], nb, D, M)
    out = _call(bank, _on_device(c["X"], False), c["coef"], labels, 5, c["seed"])
    _check_against(ref, bank, out)
    rows = out[2].cpu().numpy()
    assert not np.isin(rows[rows >= 0], bad).any()


# --------------------------------------------------------------------------- #
def _layer(F_in, F_out, M, N, **kw):
    # warm_up_flag=True: the Laplace-smoothed cluster sizes never reach zero,
    # so planted dead codewords do not raise 'Bad Init!' (vq.py:182-189)
    return LowRankGNNLayer(F_in, F_out, 0.0, M, 4, N, 0, 'vq', False, True, 0, True, True, False,
                           0, False, False, 0.5, [1, 1], True, False, True, 0.1, 'GCN', False, **kw)


@pytest.fixture(scope="module")
def layer_case():
    B, nb, D, M = SHAPES[0]
    rng = np.random.default_rng(9)
    X, st = _planted(rng, B, nb, D, M)
    g = graph.synthetic_graph(500, 5, 1800, seed=3)
    rp, cl, vl = graph.norm_adj(g, "GCN")
    b = graph.k_hop_batch(rp, cl, vl, g.N, np.arange(B))
    assert b.B == B
    return dict(x=torch.from_numpy(X).to(DEV), st=st, N=g.N, batch_A=graph.batch_to_device(b, DEV))


def _planted_layer(c, **kw):
    B, nb, D, M = SHAPES[0]
    torch.manual_seed(0)
    layer = _layer(nb * D, 8, M, c["N"], kmeans_seed=13, **kw).to(DEV)
    for k in ("emb", "ema_w", "emb_out", "cs"):
        getattr(layer._bank, k).copy_(torch.from_numpy(c["st"][k]))
    return layer


def _bank_equal(x, y):
    for (k, v), (_, w) in zip(x._bank.named_buffers(), y._bank.named_buffers()):
        assert v.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), k
    assert torch.equal(x._codes, y._codes)


def test_layer_revives_after_the_batched_call(layer_case):
    """Item 9.  revive_dead_every=1: a training forward leaves revive_result,
    bank and codes equal to a plain layer's forward followed by a direct
    bank.revive with the restated seed; codebook_health reports max(0,
    n_dead_before - revive_max) per branch."""
    B, nb, D, M = SHAPES[0]
    c = layer_case
    layer = _planted_layer(c, revive_dead_every=1).train()
    plain = _planted_layer(c).train()
    assert layer.revive_max == max(1, M // 8) and layer.revive_result is None
    out = layer(c["x"], c["batch_A"], 1.0, True)[0]
    out_plain = plain(c["x"], c["batch_A"], 1.0, True)[0]
    assert plain.revive_result is None
    n_dead_before = plain.codebook_health()[0]
    assert int(n_dead_before.min()) > layer.revive_max          # the planted half stayed dead
    direct = plain._bank.revive(c["x"], 0, nb, 1e-2, revive_ref.layer_seed(13, 1), M // 8, 1.0,
                                codes=plain._codes, batch_idx=c["batch_A"][0])
    torch.cuda.synchronize()
    for x, y in zip(layer.revive_result, direct):
        assert torch.equal(x, y)
    assert layer.revive_result[0].tolist() == [M // 8] * nb
    _bank_equal(layer, plain)
    assert torch.equal(layer.codebook_health()[0],
                       torch.clamp(n_dead_before - layer.revive_max, min=0))
    assert out.shape == out_plain.shape == (B, 8)
    # a second call draws with the second call's seed
    layer(c["x"], c["batch_A"], 1.0, True)
    plain(c["x"], c["batch_A"], 1.0, True)
    direct = plain._bank.revive(c["x"], 0, nb, 1e-2, revive_ref.layer_seed(13, 2), M // 8, 1.0,
                                codes=plain._codes, batch_idx=c["batch_A"][0])
    for x, y in zip(layer.revive_result, direct):
        assert torch.equal(x, y)
    _bank_equal(layer, plain)


def test_layer_every_n_off_and_eval(layer_case):
    """revive_dead_every=0 is the layer without the new arguments, bit for
    bit; every=2 revives on the second call only; eval() never revives."""
    c = layer_case
    off = _planted_layer(c, revive_dead_every=0).train()
    B, nb, D, M = SHAPES[0]
    torch.manual_seed(0)
    parent = _layer(nb * D, 8, M, c["N"]).to(DEV).train()      # no new argument at all
    for k in ("emb", "ema_w", "emb_out", "cs"):
        getattr(parent._bank, k).copy_(torch.from_numpy(c["st"][k]))
    o1 = off(c["x"], c["batch_A"], 1.0, True)[0]
    o2 = parent(c["x"], c["batch_A"], 1.0, True)[0]
    assert torch.equal(o1, o2) and off.revive_result is None
    _bank_equal(off, parent)

    two = _planted_layer(c, revive_dead_every=2).train()
    two(c["x"], c["batch_A"], 1.0, True)
    assert two.revive_result is None
    two(c["x"], c["batch_A"], 1.0, True)
    assert two.revive_result is not None and int(two.revive_result[0].min()) == M // 8

    ev = _planted_layer(c, revive_dead_every=1).eval()
    ref = _planted_layer(c).eval()
    with torch.no_grad():
        ev(c["x"], c["batch_A"], 1.0, True)
        ref(c["x"], c["batch_A"], 1.0, True)
    assert ev.revive_result is None
    _bank_equal(ev, ref)
