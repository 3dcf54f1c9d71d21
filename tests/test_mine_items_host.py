"""Host side of same-item mining (item_alignment_amd.retrieval, mine_items.py): the three loaders on files written here, the refusals of
ragged rows and of probabilities in place of embeddings, recall_at_k on a hand-made case, the binding entries of the kernels and their
argument checks (which run before any launch), and the refusals of the command line -- nothing is written on a refusal."""
import json
import os

import pytest
import torch

import mine_items
from item_alignment_amd import _lib
from item_alignment_amd import retrieval as R


def _jsonl(path, recs):
    with open(path, "w") as f:
        for r in recs:
            f.write(json.dumps(r) + "\n")


def _pred(src, se, tgt, te):
    return {"src_item_id": src, "src_item_emb": str(se), "tgt_item_id": tgt, "tgt_item_emb": str(te), "threshold": 0.5}


def test_pt_loader_with_and_without_ids(tmp_path):
    x = torch.arange(12, dtype=torch.float32).reshape(4, 3)
    torch.save(x, tmp_path / "feature_matrix.pt")
    (tmp_path / "entity2id.txt").write_text("a\t0\nb\t1\n\nc\t2\nd\t3\n")
    ids, got, differing = R.load_embeddings(str(tmp_path / "feature_matrix.pt"), str(tmp_path / "entity2id.txt"))
    assert ids == ["a", "b", "c", "d"] and torch.equal(got, x) and differing == 0
    ids, _, _ = R.load_embeddings(str(tmp_path / "feature_matrix.pt"))
    assert ids == ["0", "1", "2", "3"]
    (tmp_path / "short.txt").write_text("a\t0\n")
    with pytest.raises(ValueError, match="1 ids for the 4 rows"):
        R.load_embeddings(str(tmp_path / "feature_matrix.pt"), str(tmp_path / "short.txt"))
    torch.save(torch.zeros(4, 1), tmp_path / "probs.pt")
    with pytest.raises(ValueError, match="no embeddings"):
        R.load_embeddings(str(tmp_path / "probs.pt"))


def test_json_loader(tmp_path):
    (tmp_path / "image_embedding.json").write_text(json.dumps({"i9": [1.0, 2.0, 3.5], "i2": [0.0, -1.0, 4.0]}))
    ids, x, differing = R.load_embeddings(str(tmp_path / "image_embedding.json"))
    assert ids == ["i9", "i2"] and x.tolist() == [[1.0, 2.0, 3.5], [0.0, -1.0, 4.0]] and differing == 0
    (tmp_path / "ragged.json").write_text(json.dumps({"i9": [1.0, 2.0, 3.5], "i2": [0.0, -1.0]}))
    with pytest.raises(ValueError, match="item i2"):
        R.load_embeddings(str(tmp_path / "ragged.json"))


def test_jsonl_loader_first_occurrence_wins_and_counts_the_rest(tmp_path):
    p = str(tmp_path / "deepAI_result_x.jsonl")
    _jsonl(p, [_pred("a", [1.0, 0.0], "b", [0.0, 1.0]),
               _pred("a", [1.0, 0.0], "c", [0.5, 0.5]),        # a again, the same: not counted
               _pred("b", [0.0, 2.0], "a", [3.0, 0.0])])       # b and a again, both different: counted
    ids, x, differing = R.load_embeddings(p)
    assert ids == ["a", "b", "c"] and x.tolist() == [[1.0, 0.0], [0.0, 1.0], [0.5, 0.5]] and differing == 2


def test_jsonl_loader_refuses_ragged_rows_and_probabilities_naming_the_line(tmp_path):
    p = str(tmp_path / "ragged.jsonl")
    _jsonl(p, [_pred("a", [1.0, 0.0], "b", [0.0, 1.0]), _pred("c", [1.0, 0.0, 2.0], "d", [0.0, 1.0])])
    with pytest.raises(ValueError, match="line 2"):
        R.load_embeddings(p)
    p = str(tmp_path / "one_tower.jsonl")
    _jsonl(p, [_pred("a", [0.3], "b", [0.7])])
    with pytest.raises(ValueError, match="line 1.*probabilities"):
        R.load_embeddings(p)
    p = str(tmp_path / "broken.jsonl")
    _jsonl(p, [_pred("a", [1.0, 0.0], "b", [0.0, 1.0]), {"src_item_id": "c"}])
    with pytest.raises(ValueError, match="line 2"):
        R.load_embeddings(p)
    with pytest.raises(ValueError, match="unknown embedding format"):
        R.load_embeddings(str(tmp_path / "x.npy"))


def test_recall_at_k_on_a_hand_made_case():
    ids = ["a", "b", "c", "d"]
    idx = torch.tensor([[1, 2], [0, 3], [3, -1], [2, 1]])      # a: b c;  b: a d;  c: d;  d: c b
    pairs = [("a", "b", 1),     # rank 1
             ("a", "c", 1),     # rank 2
             ("b", "c", 1),     # absent
             ("c", "a", 0),     # a negative: not counted
             ("a", "zz", 1),    # unknown tgt
             ("yy", "a", 1)]    # unknown src
    recall, mrr, used, skipped = R.recall_at_k(idx, ids, pairs)
    assert (used, skipped) == (3, 2)
    assert recall == pytest.approx(2 / 3) and mrr == pytest.approx((1 + 0.5 + 0) / 3)
    # foreign queries: query row 0 is item "q0"
    recall, mrr, used, skipped = R.recall_at_k(idx[:1], ids, [("q0", "c", 1), ("a", "b", 1)], query_ids=["q0"])
    assert (recall, mrr, used, skipped) == (1.0, 0.5, 1, 1)
    assert R.recall_at_k(idx, ids, []) == (0.0, 0.0, 0, 0)


def test_index_refuses_an_unknown_metric():
    with pytest.raises(ValueError, match="cosine"):
        R.ItemIndex(torch.zeros(3, 4), metric="l2")


def test_binding_entries_and_argument_checks_before_any_launch():
    lib = _lib.load()
    assert lib.ia_sim_row_pitch(1) == 64 and lib.ia_sim_row_pitch(64) == 64 and lib.ia_sim_row_pitch(65) == 128
    assert lib.ia_sim_row_pitch(768) == 768 and lib.ia_sim_row_pitch(0) == 0
    ws = lib.ia_sim_topk_workspace_bytes
    assert ws(4096, 768, 258211, 10, 0) >= 4096 * 10 * 8
    assert ws(4096, 768, 258211, 10, 1) == 4096 * 10 * 8
    assert ws(0, 768, 100, 10, 0) == 0 and ws(10, 768, 0, 10, 0) == 0
    assert ws(10, 768, 100, 0, 0) == 0 and ws(10, 768, 100, 65, 0) == 0 and ws(10, 0, 100, 10, 0) == 0
    p = 0x1000                                                 # a pointer that is never followed: every call below is refused first
    ARG = -1
    ok = dict(q=p, cand=p, B=4, D=8, n=5, skip=None, k=2, ms=0, idx=p, score=p, ws=p, wsb=1 << 20)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ia_sim_topk(a["q"], a["cand"], a["B"], a["D"], a["n"], a["skip"], a["k"], a["ms"], a["idx"], a["score"], a["ws"], a["wsb"], None)
    for bad in (dict(q=None), dict(cand=None), dict(idx=None), dict(score=None), dict(ws=None), dict(k=0), dict(k=65), dict(D=0), dict(B=-1),
                dict(n=-1), dict(ms=-1), dict(wsb=8), dict(q=p + 2)):
        assert call(**bad) == ARG, bad
    assert lib.ia_sim_topk(p, p, 0, 8, 5, None, 2, 0, p, p, None, 0, None) == 0      # B == 0: nothing to do, no launch
    rows = lib.ia_sim_rows_bf16
    assert rows(None, 8, 4, 8, 0, p, None) == ARG and rows(p, 8, 4, 8, 0, None, None) == ARG
    assert rows(p, 7, 4, 8, 0, p, None) == ARG and rows(p, 8, -1, 8, 0, p, None) == ARG and rows(p, 8, 4, 0, 0, p, None) == ARG
    assert rows(p, 8, 4, 8, 2, p, None) == ARG
    assert rows(p, 8, 0, 8, 1, p, None) == 0


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture()
def files(tmp_path):
    torch.save(torch.eye(4, 6), tmp_path / "cat.pt")
    (tmp_path / "ids.txt").write_text("a\nb\nc\nd\n")
    (tmp_path / "q.json").write_text(json.dumps({"x": [1.0, 0.0, 0.0]}))
    _jsonl(str(tmp_path / "pairs.jsonl"), [{"src_item_id": "a", "tgt_item_id": "b", "item_label": "1"}])
    return tmp_path


def _refused(files, extra, match, **over):
    out = files / "out.jsonl"
    argv = {"--embeddings": str(files / "cat.pt"), "--ids_file": str(files / "ids.txt"), "--output_file": str(out)}
    argv.update(over)
    flat = [a for kv in argv.items() if kv[1] is not None for a in kv] + extra
    with pytest.raises(SystemExit, match=match):
        mine_items.main(flat)
    assert not out.exists()


def test_cli_refusals_write_nothing(files):
    _refused(files, ["--metric", "l2"], "use cosine or ip")
    _refused(files, ["--top_k", "0"], "between 1 and 64")
    _refused(files, ["--top_k", "65"], "between 1 and 64")
    _refused(files, ["--batch_size", "0"], "positive batch size")
    _refused(files, [], "does not exist", **{"--embeddings": str(files / "nope.pt")})
    _refused(files, [], "does not exist", **{"--ids_file": str(files / "nope.txt")})
    _refused(files, ["--pairs_file", str(files / "nope.jsonl")], "does not exist")
    _refused(files, ["--query_ids_file", str(files / "ids.txt")], "needs that flag")
    _refused(files, [], "unknown embedding format", **{"--embeddings": str(files / "ids.txt"), "--ids_file": None})
    _refused(files, ["--query_embeddings", str(files / "q.json")], "rows of 3 numbers, the catalogue's have 6")
    (files / "short.txt").write_text("a\n")
    _refused(files, [], "1 ids for the 4 rows", **{"--ids_file": str(files / "short.txt")})
    (files / "bad_pairs.jsonl").write_text('{"src_item_id": "a"}\n')
    _refused(files, ["--pairs_file", str(files / "bad_pairs.jsonl")], "line 1")


def test_cli_without_a_gpu_is_refused(files, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    _refused(files, [], "runs on the GPU")


def test_cli_without_required_flags_exits(files):
    with pytest.raises(SystemExit):
        mine_items.main(["--output_file", str(files / "out.jsonl")])
    assert not os.path.exists(files / "out.jsonl")
