"""mine_items.py --index ivf end to end on the GPU, on the 300-item catalogue with 20 planted near-duplicate pairs of
test_mine_items_cli_gpu.py: every list probed writes the bytes of --index flat; with two probes a planted twin that shares its twin's
list is found; --index_file is written once and read afterwards; --recall_check prints its line."""
import contextlib
import io
import json
import re

import pytest
import torch

import mine_items

pytestmark = pytest.mark.gpu

N, D, PAIRS = 300, 48, 20


@pytest.fixture(scope="module")
def catalogue(tmp_path_factory):
    d = tmp_path_factory.mktemp("mine_ivf")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, D, generator=g)
    for p in range(PAIRS):                                     # item 2p + 1 = item 2p + small noise
        x[2 * p + 1] = x[2 * p] + 0.02 * torch.randn(D, generator=g)
    ids = [f"item{i:03d}" for i in range(N)]
    torch.save(x, d / "feature_matrix.pt")
    (d / "entity2id.txt").write_text("".join(f"{n}\t{i}\n" for i, n in enumerate(ids)))
    return d, x, ids


def _run(d, out, *extra):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        mine_items.main(["--embeddings", str(d / "feature_matrix.pt"), "--ids_file", str(d / "entity2id.txt"), "--output_file", str(d / out),
                         "--batch_size", "128"] + list(extra))
    return (d / out).read_text(), buf.getvalue()


def test_every_list_probed_writes_the_bytes_of_the_flat_index(gpu, catalogue):
    d, x, ids = catalogue
    flat, said = _run(d, "flat.jsonl", "--index", "flat")
    assert "ivf" not in said
    ivf, said = _run(d, "ivf.jsonl", "--index", "ivf", "--nlist", "8", "--nprobe", "8")
    assert ivf == flat
    assert re.search(r"^ivf nlist=8 empty=\d+ list length min=\d+ median=\d+ max=\d+$", said, re.M), said
    rescored = _run(d, "ivf_r.jsonl", "--index", "ivf", "--nlist", "8", "--nprobe", "8", "--rescore", "--min_score", "0.9")[0]
    assert rescored == _run(d, "flat_r.jsonl", "--rescore", "--min_score", "0.9")[0]


def test_index_file_is_written_once_then_read_and_twins_sharing_a_list_are_found(gpu, catalogue):
    d, x, ids = catalogue
    path = d / "index.pt"
    first, _ = _run(d, "ivf2.jsonl", "--index", "ivf", "--nlist", "8", "--nprobe", "2", "--index_file", str(path))
    saved = torch.load(path)
    assert saved["N"] == N and saved["D"] == D and saved["nlist"] == 8 and saved["metric"] == "cosine" and saved["centroids"].shape == (8, D)
    rows = [json.loads(l) for l in first.splitlines()]
    shared = 0
    for p in range(2 * PAIRS):
        if saved["assignment"][p] == saved["assignment"][p ^ 1]:
            shared += 1
            assert ids[p ^ 1] in rows[p]["neighbours"], ("a twin in the probed list is missed", p)
    assert shared > 0
    stamp = path.stat().st_mtime_ns
    # a second run reads the file: flags that would train another index (another seed, no k-means) change nothing
    second, _ = _run(d, "ivf3.jsonl", "--index", "ivf", "--nprobe", "2", "--index_file", str(path), "--seed", "5", "--kmeans_iters", "0")
    assert second == first and path.stat().st_mtime_ns == stamp
    with pytest.raises(SystemExit, match="--nlist 5.*holds 8"):
        _run(d, "ivf4.jsonl", "--index", "ivf", "--nlist", "5", "--index_file", str(path))
    torch.save(x[:, :40].clone(), d / "narrow.pt")
    with pytest.raises(SystemExit, match="D = 48.*D = 40"):
        mine_items.main(["--embeddings", str(d / "narrow.pt"), "--output_file", str(d / "narrow.jsonl"), "--index", "ivf", "--index_file", str(path)])


def test_recall_check_prints_its_line(gpu, catalogue):
    d, x, ids = catalogue
    _, said = _run(d, "ivf5.jsonl", "--index", "ivf", "--nlist", "8", "--nprobe", "8", "--recall_check", "64")
    assert "ivf_recall@10=1.0000 over 64 queries (nprobe=8, nlist=8)" in said, said
    _, said = _run(d, "ivf6.jsonl", "--index", "ivf", "--nlist", "8", "--nprobe", "1", "--recall_check", "64", "--top_k", "5")
    m = re.search(r"ivf_recall@5=([01]\.\d{4}) over 64 queries \(nprobe=1, nlist=8\)", said)
    assert m and 0.0 <= float(m.group(1)) <= 1.0, said
    torch.save(x[:70].clone(), d / "queries.pt")
    _, said = _run(d, "ivf7.jsonl", "--index", "ivf", "--nlist", "8", "--nprobe", "8", "--recall_check", "64", "--query_embeddings", str(d / "queries.pt"))
    assert "ivf_recall@10=1.0000 over 64 queries (nprobe=8, nlist=8)" in said, said
