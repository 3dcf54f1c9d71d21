"""mine_items.py end to end on the GPU: a 300-item catalogue with 20 planted near-duplicate pairs, read as feature_matrix.pt + ids file
and as image_embedding.json; foreign queries; --rescore against torch's fp32 dots; --min_score."""
import contextlib
import io
import json

import pytest
import torch

import mine_items

pytestmark = pytest.mark.gpu

N, D, PAIRS = 300, 48, 20


@pytest.fixture(scope="module")
def catalogue(tmp_path_factory):
    d = tmp_path_factory.mktemp("mine")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, D, generator=g)
    for p in range(PAIRS):                                     # item 2p + 1 = item 2p + small noise
        x[2 * p + 1] = x[2 * p] + 0.02 * torch.randn(D, generator=g)
    ids = [f"item{i:03d}" for i in range(N)]
    torch.save(x, d / "feature_matrix.pt")
    (d / "entity2id.txt").write_text("".join(f"{n}\t{i}\n" for i, n in enumerate(ids)))
    (d / "image_embedding.json").write_text(json.dumps({n: x[i].tolist() for i, n in enumerate(ids)}))
    with open(d / "item_valid_pair.jsonl", "w") as f:
        for p in range(PAIRS):
            f.write(json.dumps({"src_item_id": ids[2 * p], "tgt_item_id": ids[2 * p + 1], "item_label": "1"}) + "\n")
            f.write(json.dumps({"src_item_id": ids[2 * p + 1], "tgt_item_id": ids[2 * p], "item_label": "1"}) + "\n")
        f.write(json.dumps({"src_item_id": ids[0], "tgt_item_id": ids[100], "item_label": "0"}) + "\n")
        f.write(json.dumps({"src_item_id": ids[0], "tgt_item_id": "elsewhere", "item_label": "1"}) + "\n")
    return d, x, ids


def _lines(path):
    return [json.loads(l) for l in open(path)]


@pytest.fixture(scope="module")
def plain(gpu, catalogue):
    """the run every test compares with: the .pt catalogue, the defaults but for three kernel calls instead of one"""
    d, x, ids = catalogue
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mine_items.main(["--embeddings", str(d / "feature_matrix.pt"), "--ids_file", str(d / "entity2id.txt"), "--output_file",
                         str(d / "pt.jsonl"), "--pairs_file", str(d / "item_valid_pair.jsonl"), "--batch_size", "128"])
    return _lines(d / "pt.jsonl"), buf.getvalue()


def test_both_formats_give_the_same_lists_and_find_the_planted_twins(gpu, catalogue, plain):
    d, x, ids = catalogue
    out = plain[1]
    assert "recall@10=1.0" in out and f"positives={2 * PAIRS} skipped=1" in out, out
    mine_items.main(["--embeddings", str(d / "image_embedding.json"), "--output_file", str(d / "json.jsonl")])
    assert (d / "pt.jsonl").read_text() == (d / "json.jsonl").read_text()
    rows = plain[0]
    assert [r["item_id"] for r in rows] == ids
    for i, r in enumerate(rows):
        assert len(r["neighbours"]) == len(r["scores"]) == 10 and r["item_id"] not in r["neighbours"]
        assert r["scores"] == sorted(r["scores"], reverse=True)
        if i < 2 * PAIRS:
            assert r["neighbours"][0] == ids[i ^ 1] and r["scores"][0] > 0.99


def test_foreign_queries_keep_identical_rows(gpu, catalogue):
    d, x, ids = catalogue
    torch.save(x[[7, 250]].clone(), d / "queries.pt")
    (d / "query_ids.txt").write_text("q7\nq250\n")
    mine_items.main(["--embeddings", str(d / "feature_matrix.pt"), "--ids_file", str(d / "entity2id.txt"), "--query_embeddings",
                     str(d / "queries.pt"), "--query_ids_file", str(d / "query_ids.txt"), "--top_k", "3", "--output_file", str(d / "q.jsonl")])
    rows = _lines(d / "q.jsonl")
    assert [r["item_id"] for r in rows] == ["q7", "q250"]
    assert rows[0]["neighbours"][:2] == [ids[7], ids[6]] and rows[1]["neighbours"][0] == ids[250]
    assert abs(rows[1]["scores"][0] - 1.0) < 2 ** -7


def test_rescore_reports_fp32_dots(gpu, catalogue, plain):
    d, x, ids = catalogue
    mine_items.main(["--embeddings", str(d / "feature_matrix.pt"), "--ids_file", str(d / "entity2id.txt"), "--rescore", "--top_k", "5",
                     "--output_file", str(d / "rescored.jsonl")])
    xn = torch.nn.functional.normalize(x, dim=1)
    row_of = {n: i for i, n in enumerate(ids)}
    for i, r in enumerate(_lines(d / "rescored.jsonl")):
        nb = [row_of[n] for n in r["neighbours"]]
        want = (xn[nb] * xn[i]).sum(-1)
        assert (torch.tensor(r["scores"]) - want).abs().max() <= 1e-6
        assert r["scores"] == sorted(r["scores"], reverse=True)
        assert sorted(r["neighbours"]) == sorted(plain[0][i]["neighbours"][:5])      # the same ids as without --rescore


def test_min_score_drops_entries(gpu, catalogue):
    d, x, ids = catalogue
    mine_items.main(["--embeddings", str(d / "feature_matrix.pt"), "--ids_file", str(d / "entity2id.txt"), "--min_score", "0.9",
                     "--output_file", str(d / "min.jsonl")])
    rows = _lines(d / "min.jsonl")
    assert len(rows) == N
    for i, r in enumerate(rows):
        assert r["neighbours"] == ([ids[i ^ 1]] if i < 2 * PAIRS else []) and all(s >= 0.9 for s in r["scores"])
