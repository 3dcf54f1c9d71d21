"""Writes tests/golden/coca/collate_coca.json from the reference's own MultimodalDataset and collate_coca (src/data/data.py:872-915, :15-34).

    python tools/gen_golden_coca_collate.py <reference checkout>

The reference's data module is imported under the stubs of oracle/gen_collates.py (jieba, timm's create_transform, the tokenizer enums)
with the fake tokenizer of tests/fake_tokenizer.py, so the fixture does not depend on the installed transformers version.  Three
settings on the same six seeded rows (item_id, title, pvs, image path): title only, pvs only, title + pvs.  The stubbed transform
produces no image, so -- as gen_collates.py does for collate_coca_pair -- the records get hand-made image tensors; in the third setting
item 3 stays without one (its file is "missing") and the collate must drop it.  What is pinned is the text of every record, the tuple
order, the dtypes and the dropping.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = (("title_only", 8, None, None), ("pvs_only", None, 12, None), ("title_pvs_one_image_missing", 8, 12, 3))


def main(reference):
    sys.path.insert(0, ROOT)
    from oracle import gen_collates as G
    if not os.path.realpath(G.D.__file__).startswith(os.path.realpath(reference)):
        raise SystemExit(f"oracle/gen_collates.py imported the reference from {G.D.__file__}, not from {reference}")
    rs = np.random.RandomState(23)
    tk = G.FakeBertTokenizer()
    rows = [[r[1] + f"_{i}", r[3], r[4], f"img_{i}.png"] for i, r in enumerate(G.text_rows(rs, 6))]

    def img(k):
        return torch.arange(3 * 4 * 4, dtype=torch.float32).reshape(3, 4, 4) + 100 * k

    out = {"bos_token": tk.bos_token, "cases": []}
    for name, max_seq_len, max_seq_len_pv, missing in SETTINGS:
        ds = G.D.MultimodalDataset([tuple(r[:3]) + ("/nonexistent/" + r[3],) for r in rows], 16, False, tk, max_seq_len,
                                   max_seq_len_pv=max_seq_len_pv)
        recs = []
        for i in range(len(ds)):
            rec = ds[i]
            assert "image" not in rec
            if i != missing:
                rec["image"] = img(i)
            recs.append(rec)
        out["cases"].append({"name": name, "kw": dict(image_size=16, is_training=False, max_seq_len=max_seq_len, max_seq_len_pv=max_seq_len_pv),
                             "rows": rows, "missing_image": [] if missing is None else [missing], "records": G.jsonable(recs),
                             "batch": G.jsonable(G.D.collate_coca(recs))})
    path = os.path.join(ROOT, "tests", "golden", "coca", "collate_coca.json")
    with open(path, "w", encoding="utf8") as f:
        json.dump(out, f, ensure_ascii=False, sort_keys=True)
    print("wrote", path, len(out["cases"]), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
