"""Host side of the inverted-file index: the refusals the new flags of mine_items.py add (nothing is written on a refusal), and the
argument checks of ia_sim_topk_groups, ia_sim_topk_fold and ia_sim_centroid_sums, which run before any launch, so the library answers
them without a GPU."""
import pytest
import torch

import mine_items
from item_alignment_amd import _lib


@pytest.fixture()
def files(tmp_path):
    torch.save(torch.eye(4, 6), tmp_path / "cat.pt")
    return tmp_path


def _refused(files, extra, match):
    out = files / "out.jsonl"
    with pytest.raises(SystemExit, match=match):
        mine_items.main(["--embeddings", str(files / "cat.pt"), "--output_file", str(out)] + extra)
    assert not out.exists()


def test_ivf_flags_are_refused_without_the_ivf_index(files):
    for flag, value in (("nlist", "2"), ("nprobe", "2"), ("train_size", "4"), ("kmeans_iters", "3"), ("seed", "1"),
                        ("index_file", str(files / "index.pt")), ("recall_check", "2")):
        _refused(files, [f"--{flag}", value], f"--{flag}.*--index ivf")
        _refused(files, ["--index", "flat", f"--{flag}", value], f"--{flag}.*--index ivf")
    assert not (files / "index.pt").exists()


def test_ivf_flags_out_of_range_are_refused_naming_the_flag(files, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)         # each refusal below comes before the GPU is asked for
    _refused(files, ["--index", "hnsw"], "--index hnsw")
    _refused(files, ["--index", "ivf", "--nlist", "0"], "--nlist 0")
    _refused(files, ["--index", "ivf", "--nlist", "5"], "--nlist 5.*N = 4")
    _refused(files, ["--index", "ivf", "--nprobe", "0"], "--nprobe 0")
    _refused(files, ["--index", "ivf", "--recall_check", "0"], "--recall_check 0")
    _refused(files, ["--index", "ivf", "--train_size", "0"], "--train_size 0")
    _refused(files, ["--index", "ivf", "--kmeans_iters", "-1"], "--kmeans_iters -1")
    _refused(files, ["--index", "ivf", "--nlist", "4"], "runs on the GPU")  # in range: only the GPU is missing


P = 0x1000                                                     # a pointer that is never followed: every call below is refused first
ARG = -1


def test_topk_groups_argument_checks_before_any_launch():
    lib = _lib.load()
    ws = lib.ia_sim_topk_groups_workspace_bytes
    assert ws(65536, 2032, 768, 258211, 10, 0) >= 65536 * 10 * 8 + 2033 * 4
    assert ws(65536, 2032, 768, 258211, 10, 1) == (2033 * 4 + 255) // 256 * 256 + 65536 * 10 * 8
    assert ws(0, 5, 8, 100, 10, 0) == 0 and ws(10, 0, 8, 100, 10, 0) == 0
    assert ws(10, 5, 8, 0, 10, 0) > 0                                     # no candidates: the lists are still written, all unused
    assert ws(10, 5, 8, 100, 0, 0) == 0 and ws(10, 5, 8, 100, 65, 0) == 0 and ws(10, 5, 0, 100, 10, 0) == 0
    assert ws(-1, 5, 8, 100, 10, 0) == 0 and ws(10, -1, 8, 100, 10, 0) == 0 and ws(10, 5, 8, -1, 10, 0) == 0 and ws(10, 5, 8, 100, 10, -1) == 0
    ok = dict(q=P, cand=P, q_off=P, c_off=P, G=3, P=4, D=8, n=5, label=None, bits=0, skip=None, k=2, ms=0, idx=P, score=P, ws=P, wsb=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ia_sim_topk_groups(a["q"], a["cand"], a["q_off"], a["c_off"], a["G"], a["P"], a["D"], a["n"], a["label"], a["bits"], a["skip"],
                                      a["k"], a["ms"], a["idx"], a["score"], a["ws"], a["wsb"], None)
    for bad in (dict(q=None), dict(cand=None), dict(q_off=None), dict(c_off=None), dict(idx=None), dict(score=None), dict(ws=None),
                dict(k=0), dict(k=65), dict(D=0), dict(P=-1), dict(G=-1), dict(n=-1), dict(ms=-1), dict(wsb=8),
                dict(q=P + 2), dict(cand=P + 8), dict(q_off=P + 4), dict(c_off=P + 4), dict(skip=P + 4), dict(idx=P + 4), dict(score=P + 2),
                dict(ws=P + 8), dict(label=P), dict(label=P, bits=16), dict(bits=32), dict(label=P + 4, bits=64), dict(label=P + 2, bits=32)):
        assert call(**bad) == ARG, bad
    assert call(G=0, ws=None, wsb=0) == 0 and call(P=0, ws=None, wsb=0) == 0          # nothing to do, no launch


def test_fold_and_centroid_sums_argument_checks_before_any_launch():
    lib = _lib.load()
    fold, sums = lib.ia_sim_topk_fold, lib.ia_sim_centroid_sums
    for bad in ((None, P, 4, P, 2, 3, 2, P, P), (P, None, 4, P, 2, 3, 2, P, P), (P, P, 4, None, 2, 3, 2, P, P), (P, P, 4, P, 2, 3, 2, None, P),
                (P, P, 4, P, 2, 3, 2, P, None), (P, P, -1, P, 2, 3, 2, P, P), (P, P, 4, P, -1, 3, 2, P, P), (P, P, 4, P, 2, 0, 2, P, P),
                (P, P, 4, P, 2, 3, 0, P, P), (P, P, 4, P, 2, 3, 65, P, P), (P + 4, P, 4, P, 2, 3, 2, P, P), (P, P + 2, 4, P, 2, 3, 2, P, P),
                (P, P, 4, P + 4, 2, 3, 2, P, P), (P, P, 4, P, 2, 3, 2, P + 4, P), (P, P, 4, P, 2, 3, 2, P, P + 2)):
        assert fold(*bad, None) == ARG, bad
    assert fold(P, P, 4, P, 0, 3, 2, P, P, None) == 0                     # B == 0: no launch
    for bad in ((None, 4, 8, P, 4, P, 2, P, P), (P, 4, 8, None, 4, P, 2, P, P), (P, 4, 8, P, 4, None, 2, P, P), (P, 4, 8, P, 4, P, 2, None, P),
                (P, 4, 8, P, 4, P, 2, P, None), (P, -1, 8, P, 4, P, 2, P, P), (P, 4, 0, P, 4, P, 2, P, P), (P, 4, 8, P, -1, P, 2, P, P),
                (P, 4, 8, P, 4, P, -1, P, P), (P + 1, 4, 8, P, 4, P, 2, P, P), (P, 4, 8, P + 4, 4, P, 2, P, P), (P, 4, 8, P, 4, P + 4, 2, P, P),
                (P, 4, 8, P, 4, P, 2, P + 2, P), (P, 4, 8, P, 4, P, 2, P, P + 4)):
        assert sums(*bad, None) == ARG, bad
    assert sums(P, 4, 8, P, 4, P, 0, P, P, None) == 0                     # no lists: no launch
