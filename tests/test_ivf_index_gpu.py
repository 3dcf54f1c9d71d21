"""retrieval.IVFItemIndex on the GPU against retrieval.ItemIndex and tests/ivf_reference.py.

With every list probed the inverted-file index is the exact index: ids equal, scores bit-equal.  With fewer probes the result is the
exact selection over the probed lists (select_probed for the probes search() reports): bit for bit on exact operands, under check_topk
on random rows.  Probes are nested in nprobe, so the number of exact-list entries found does not decrease with nprobe and is complete at
nprobe == nlist -- a property of nested candidate sets; no recall threshold is asserted."""
import numpy as np
import pytest
import torch

import ivf_reference as IR
import simtopk_reference as SR

pytestmark = pytest.mark.gpu

N = 1500


def _R():
    from item_alignment_amd import retrieval
    return retrieval


def _clustered(D, n=N, centres=30, seed=0):
    g = torch.Generator().manual_seed(seed + D)
    c = torch.nn.functional.normalize(torch.randn(centres, D, generator=g), dim=1)
    return c[torch.randint(0, centres, (n,), generator=g)] + 0.05 * torch.randn(n, D, generator=g)


def _same(got, want, what):
    assert torch.equal(got[0], want[0]), (what, "ids", (got[0] != want[0]).nonzero()[:4])
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (what, "scores")


@pytest.fixture(scope="module")
def exact(gpu):
    """per D: the rows, foreign queries, and the exact index's answers, computed once"""
    R = _R()
    out = {}
    for D in (72, 200):
        x, q = _clustered(D), _clustered(D, n=130, seed=5)
        flat = R.ItemIndex(x)
        out[D] = dict(x=x, q=q, own={k: flat.search(k=k) for k in (10, 64)}, foreign={k: flat.search(q, k=k) for k in (10, 64)})
    return out


@pytest.mark.parametrize("nlist", [1, 7, 40])
@pytest.mark.parametrize("D", [72, 200])
def test_every_list_probed_equals_the_exact_index(gpu, exact, D, nlist):
    R = _R()
    e = exact[D]
    index = R.IVFItemIndex(e["x"], nlist=nlist, nprobe=nlist, kmeans_iters=3)
    IR.check_layout(index.row_id, index.inv, index.list_off, index.assignment)
    for k in (10, 64):
        _same(index.search(k=k, batch_size=600), e["own"][k], ("own", D, nlist, k))
        _same(index.search(e["q"], k=k), e["foreign"][k], ("foreign", D, nlist, k))
    _same(index.search(k=10, nprobe=10 ** 6), e["own"][10], "nprobe is clamped to nlist")


def test_lists_on_tile_edges_with_an_explicit_assignment(gpu, exact):
    """list 0 empty, list 1 a single row, list 2 of 129 rows, the rest in list 3"""
    R = _R()
    e = exact[72]
    g = torch.Generator().manual_seed(1)
    perm = torch.randperm(N, generator=g)
    assignment = torch.full((N,), 3)
    assignment[perm[0]] = 1
    assignment[perm[1:130]] = 2
    centroids = torch.nn.functional.normalize(torch.randn(4, 72, generator=g), dim=1)
    index = R.IVFItemIndex(e["x"], centroids=centroids, assignment=assignment, nprobe=4)
    IR.check_layout(index.row_id, index.inv, index.list_off, assignment)
    assert index.list_sizes().tolist() == [0, 1, 129, N - 130]
    assert index.summary() == f"ivf nlist=4 empty=1 list length min=0 median=1 max={N - 130}"
    for k in (10, 64):
        _same(index.search(k=k), e["own"][k], ("edges", k))
        _same(index.search(e["q"], k=k), e["foreign"][k], ("edges, foreign", k))


@pytest.mark.parametrize("k", [10, 64])
def test_exact_operands_with_fewer_probes_bit_equal(gpu, k):
    """whole numbers in [-4, 4], metric ip, whole-number centroids: every score is exact, the rows are full of ties and duplicates"""
    R = _R()
    n, D, nlist = 1200, 72, 9
    g = torch.Generator().manual_seed(k)
    x = torch.randint(-4, 5, (60, D), generator=g).float()[torch.randint(0, 60, (n,), generator=g)]
    q = torch.randint(-4, 5, (130, D), generator=g).float()
    centroids = torch.randint(-4, 5, (nlist, D), generator=g).float()
    assignment = torch.randint(0, nlist, (n,), generator=g)    # duplicates of a row land in different lists
    index = R.IVFItemIndex(x, metric="ip", centroids=centroids, assignment=assignment)
    own, foreign = SR.scores_fp64(x, x).astype(np.float32), SR.scores_fp64(q, x).astype(np.float32)
    for nprobe in (1, 3, 9):
        idx, score, probes = index.search(k=k, nprobe=nprobe, return_probes=True, batch_size=500)
        assert probes.shape == (n, nprobe) and all(len(set(p)) == nprobe for p in probes.tolist())
        want = IR.select_probed(own, assignment, probes, k, skip=np.arange(n))
        assert np.array_equal(idx.numpy(), want[0]) and np.array_equal(score.numpy().view(np.int32), want[1].view(np.int32)), ("own", nprobe)
        idx, score, probes = index.search(q, k=k, nprobe=nprobe, return_probes=True)
        want = IR.select_probed(foreign, assignment, probes, k)
        assert np.array_equal(idx.numpy(), want[0]) and np.array_equal(score.numpy().view(np.int32), want[1].view(np.int32)), ("foreign", nprobe)
        idx, score = index.search(q, k=k, nprobe=nprobe, exclude_self=True)      # catalogue row i is kept from query i
        want = IR.select_probed(foreign, assignment, probes, k, skip=np.arange(130))
        assert np.array_equal(idx.numpy(), want[0]), ("foreign, exclude_self", nprobe)


def test_random_rows_with_fewer_probes_and_nested_probes(gpu, exact):
    R = _R()
    e = exact[200]
    index = R.IVFItemIndex(e["x"], nlist=40, kmeans_iters=5)
    rows = index.rows[index.inv]                               # the bf16 rows in original order
    s64 = SR.scores_fp64(rows.float(), rows.float())
    bars = SR.bar(rows.float(), rows.float(), rows.shape[1])
    k = 10
    exact_sets = [set(r) for r in e["own"][k][0].tolist()]
    found_before, probes_before = np.zeros(N, np.int64), None
    for nprobe in (1, 4, 16, 40):
        idx, score, probes = index.search(k=k, nprobe=nprobe, return_probes=True)
        if probes_before is not None:
            assert torch.equal(probes[:, :probes_before.shape[1]], probes_before), "probes are nested in nprobe"
        allowed = (index.assignment.numpy()[None, None, :] == probes.numpy()[:, :, None]).any(1)      # [query, row]: the row's list is probed
        for b in range(N):                                     # check_topk over the rows of the probed lists alone
            cols = np.nonzero(allowed[b])[0]
            used = idx[b][idx[b] >= 0].numpy()
            assert allowed[b, used].all(), ("a row of an unprobed list is returned", nprobe, b)
            local = np.full(k, -1, np.int64)
            local[:len(used)] = np.searchsorted(cols, used)
            own = int(np.searchsorted(cols, b))                # the query's own row among them (it is, when its list is probed)
            SR.check_topk(local[None], score[b][None], s64[b, cols][None], bars[b, cols][None], k, [own if allowed[b, b] else -1])
        found = np.array([len(exact_sets[b] & set(r)) for b, r in enumerate(idx.tolist())])
        assert (found >= found_before).all(), ("entries of the exact list found must not decrease with nprobe", nprobe)
        found_before, probes_before = found, probes
    assert (found_before == k).all(), "every list probed finds the whole exact list"


@pytest.mark.parametrize("metric", ["cosine", "ip"])
def test_a_row_probes_its_own_list_first(gpu, exact, metric):
    R = _R()
    x = exact[72]["x"] * (1.0 + torch.arange(N)[:, None] % 5)  # unequal norms: they matter for ip
    index = R.IVFItemIndex(x, metric=metric, nlist=40, kmeans_iters=3)
    idx, score, probes = index.search(k=1, nprobe=1, exclude_self=False, return_probes=True)
    assert torch.equal(probes[:, 0], index.assignment)
    # the kernel's own score of every row with itself: N groups of one query and one candidate, the same accumulator as the scan's
    every = torch.arange(N + 1)
    self_score = R.sim_topk_groups(index.rows, index.rows, every, every, 72, 1)[1][index.inv, 0].cpu()
    assert (score[:, 0] >= self_score).all()


def test_two_builds_are_equal_and_summary_counts_agree(gpu, exact):
    R = _R()
    x = exact[72]["x"]
    a, b = (R.IVFItemIndex(x, nlist=25, seed=3, train_size=900) for _ in range(2))
    assert torch.equal(a.centroids, b.centroids) and torch.equal(a.assignment, b.assignment) and torch.equal(a.row_id, b.row_id)
    assert torch.equal(a.list_off, b.list_off) and torch.equal(a.rows.view(torch.int16), b.rows.view(torch.int16))
    IR.check_layout(a.row_id, a.inv, a.list_off, a.assignment)
    c = R.IVFItemIndex(x, nlist=25, seed=4, train_size=900)
    assert not torch.equal(a.centroids, c.centroids)
    sizes = a.list_sizes()
    assert int(sizes.sum()) == N and sizes.shape == (25,)
    assert a.summary() == (f"ivf nlist=25 empty={int((sizes == 0).sum())} list length min={int(sizes.min())} "
                           f"median={int(sizes.median())} max={int(sizes.max())}")
    assert R.IVFItemIndex(x).nlist == round(4 * N ** 0.5)       # the default
    norms = a.centroids.norm(dim=1)
    assert (norms - 1).abs().max() < 2 ** -7                    # unit: a normalised sum, or a start row (unit before its bf16 rounding)


def test_save_and_load_round_trip(gpu, exact, tmp_path):
    R = _R()
    x, q = exact[72]["x"], exact[72]["q"]
    index = R.IVFItemIndex(x, nlist=20, nprobe=3)
    index.save(tmp_path / "index.pt")
    back = R.IVFItemIndex.load(tmp_path / "index.pt", x, nprobe=3)
    assert back.nlist == 20 and torch.equal(back.assignment, index.assignment) and torch.equal(back.centroids, index.centroids)
    for queries in (None, q):
        _same(back.search(queries, k=10), index.search(queries, k=10), "round trip")
    with pytest.raises(ValueError, match=f"{N}.*{N - 1}"):
        R.IVFItemIndex.load(tmp_path / "index.pt", x[:-1])
    with pytest.raises(ValueError, match="72.*64"):
        R.IVFItemIndex.load(tmp_path / "index.pt", x[:, :64])
    with pytest.raises(ValueError, match="cosine.*ip"):
        R.IVFItemIndex.load(tmp_path / "index.pt", x, metric="ip")


def test_rescore_returns_the_same_ids_and_refusals(gpu, exact):
    R = _R()
    x, q = exact[72]["x"], exact[72]["q"]
    index = R.IVFItemIndex(x, nlist=20, nprobe=5)
    for queries in (None, q):
        plain, rescored = index.search(queries, k=10), index.search(queries, k=10, rescore=True)
        assert torch.equal(plain[0].sort(dim=1)[0], rescored[0].sort(dim=1)[0])
        assert (rescored[1][:, :-1] >= rescored[1][:, 1:]).all()
    with pytest.raises(ValueError, match="keep_fp32"):
        R.IVFItemIndex(x, nlist=20, keep_fp32=False).search(k=10, rescore=True)
    for bad in (dict(k=0), dict(k=65), dict(batch_size=0), dict(nprobe=0), dict(queries=torch.zeros(3, 5))):
        with pytest.raises(ValueError):
            index.search(**bad)
    for bad in (dict(nlist=0), dict(nlist=N + 1), dict(nprobe=0), dict(nlist=10, train_size=5), dict(assignment=torch.zeros(N, dtype=torch.int64)),
                dict(centroids=torch.zeros(4, 72), assignment=torch.full((N,), 4)), dict(centroids=torch.zeros(4, 71)), dict(metric="l2")):
        with pytest.raises(ValueError):
            R.IVFItemIndex(x, **bad)
