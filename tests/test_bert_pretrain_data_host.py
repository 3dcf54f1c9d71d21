"""item_alignment_amd.data.bert_pretrain on hand-written records (CPU only): the layout facts the model depends on, label / input
consistency, the masking rates, property parsing on edge strings, truncation and reproducibility."""
import json
import math

import pytest

from bert_pretrain_tokenizer import FakePretrainTokenizer
from item_alignment_amd.data import bert_pretrain as D

TOK = FakePretrainTokenizer()
CLS, SEP, MASK = TOK.cls_token_id, TOK.sep_token_id, TOK.vocab["[MASK]"]
RECORD = {"industry_name": "手机 品牌", "cate_name": "手机", "cate_name_path": "品牌 手机", "title": "华为 手机 红色 大号 x y",
          "item_pvs": "颜色:红色;#尺码:大号;品牌:华为"}
NO_MATCH = dict(RECORD, title="a1 b2 x y a1 b2 x y", item_pvs="颜色:蓝色;尺码:小号")


def ids(text):
    return TOK.convert_tokens_to_ids(TOK.tokenize(text))


def segments(record):
    return [ids(t) for t in D.record_texts(record)]


def test_join_fills_missing_fields_and_record_texts_drops_hashes():
    d = D.join_pretraining_data({"title": "x"})
    assert d["title"] == "x" and d["industry_name"] == D.MISSING and list(d) == D.FIELD_NAMES
    assert D.record_texts(RECORD)[-1] == "颜色:红色;尺码:大号;品牌:华为"


def test_layout_of_create_input_features():
    """[CLS] ... [SEP] with label -1 and attention mask 0 on both; padding to max_seq_len + 2 with id 0, mask 0, label -1; token types
    0..3 for the fixed segments, 4 for the property segment"""
    max_len = 40
    _, masked = D.get_masked_examples(D.record_texts(RECORD), TOK, max_len, D.Rng(0))
    seg = segments(RECORD)
    n_fixed, n = sum(len(s) for s in seg[:4]), sum(len(s) for s in seg)
    assert len(masked) == 3 + 2 * 3                       # industry, category, title, and a name and a value per property
    for ex in masked:
        assert set(ex) == {"input_ids", "token_type_ids", "attention_mask", "label_ids", "next_label"} and ex["next_label"] == 1
        assert all(len(ex[k]) == max_len + 2 for k in ("input_ids", "token_type_ids", "attention_mask", "label_ids"))
# the property examples rebuild their segment as name : value ; ... and so end with a ';' the record's text lacks
        n_ex = ex["input_ids"].index(SEP) - 1
        assert n_ex in (n, n + 1) and ex["input_ids"][0] == CLS
        for p in (0, n_ex + 1):
            assert ex["attention_mask"][p] == 0 and ex["label_ids"][p] == -1 and ex["token_type_ids"][p] == 0
        assert ex["attention_mask"][1:n_ex + 1] == [1] * n_ex
        types = [t for i, s in enumerate(seg[:4]) for t in [i] * len(s)] + [4] * (n_ex - n_fixed)
        assert ex["token_type_ids"][1:n_ex + 1] == types
        tail = slice(n_ex + 2, None)
        assert set(ex["input_ids"][tail]) == {0} and set(ex["attention_mask"][tail]) == {0} and set(ex["label_ids"][tail]) == {-1}
        assert set(ex["token_type_ids"][tail]) == {0}
    assert n_fixed < max_len


def test_fixed_fields_that_fill_the_sequence_give_no_example():
    seg = segments(RECORD)
    n_fixed = sum(len(s) for s in seg[:4])
    examples = D._segments(D.record_texts(RECORD), TOK)
    assert D.create_input_features(examples, n_fixed, TOK, D.Rng(0)) == []
    assert D.create_input_features(examples, n_fixed - 1, TOK, D.Rng(0)) == []
    assert D.create_input_features(examples, n_fixed + 1, TOK, D.Rng(0)) != []
    assert D.build_examples([RECORD], TOK, n_fixed, D.Rng(0)) == []          # the collate never sees an empty example


@pytest.mark.parametrize("record", [RECORD, NO_MATCH])
def test_labels_are_the_original_ids_and_inputs_change_only_where_labelled(record):
    """label -1 wherever the position was not selected for prediction -- and there the input is the original token; a selected position's
    label is the original id whatever the input shows (the token itself, a random one, or [MASK])"""
    seg = segments(record)
    plain = [t for s in seg for t in s]
    rebuilt = plain + ids(";")               # the property examples end their segment with a ';'
    seen_changed = seen_kept = 0
    for seed in range(40):
        _, masked = D.get_masked_examples(D.record_texts(record), TOK, 60, D.Rng(seed))
        for ex in masked:
            n = ex["input_ids"].index(SEP) - 1
            flat = plain if n == len(plain) else rebuilt
            got, lab = ex["input_ids"][1:n + 1], ex["label_ids"][1:n + 1]
            assert n == len(flat)
            for g, l, o in zip(got, lab, flat):
                if l == -1:
                    assert g == o
                else:
                    assert l == o
                    seen_changed += g != o
                    seen_kept += g == o
    assert seen_changed and seen_kept


def _binomial_slack(n, p):
    """six standard deviations of a binomial count's fraction: a fair generator leaves the interval once in 5e8 tests"""
    return 6.0 * math.sqrt(p * (1 - p) / n)


def test_whole_mask_rates_are_80_10_10():
    n = 4000
    rng = D.Rng(123)
    src = ids("手机 品牌 华为")
    kept = rand = mask = 0
    for _ in range(n):
        got, lab = D.do_whole_mask(list(src), TOK, rng)
        assert lab == src
        if got == src:
            kept += 1
        elif got == [MASK] * len(src):
            mask += 1
        else:
            rand += 1
    # a random draw reproduces all three tokens with probability len(TOK)^-3 ~ 3e-7: it does not move the counts
    assert abs(kept / n - 0.8) <= _binomial_slack(n, 0.8), kept
    assert abs(rand / n - 0.1) <= _binomial_slack(n, 0.1), rand
    assert abs(mask / n - 0.1) <= _binomial_slack(n, 0.1), mask


def test_pvs_mask_rates_are_80_10_10():
    props = [[["颜色"], ["红色", "大号"]], [["品牌"], ["华为"]]]
    rng = D.Rng(5)
    kept = rand = mask = total = 0
    for _ in range(1000):
        for ex in D.do_pvs_mask(props, TOK, rng):
            sel = [i for i, l in enumerate(ex["label_ids"]) if l != -1]
            orig = TOK.convert_tokens_to_ids(ex["org_tokens"])
            assert sel and [ex["label_ids"][i] for i in sel] == [orig[i] for i in sel]
            assert all(ex["input_ids"][i] == orig[i] for i in range(len(orig)) if i not in sel)
            assert set(ex["token_type_ids"]) == {4}
            shown = [ex["input_ids"][i] for i in sel]
            total += 1
            if shown == [orig[i] for i in sel]:
                kept += 1
            elif shown == [MASK] * len(sel):
                mask += 1
            else:
                rand += 1
    assert total == 4000
    # a one-token span drawn at random equals its original once in len(TOK) = 151 draws: 0.1 / 151 moves from `rand` to `kept`
    assert abs(kept / total - 0.8) <= _binomial_slack(total, 0.8) + 0.1 / len(TOK), kept
    assert abs(rand / total - 0.1) <= _binomial_slack(total, 0.1) + 0.1 / len(TOK), rand
    assert abs(mask / total - 0.1) <= _binomial_slack(total, 0.1), mask


def test_title_mask_selects_15_percent_without_spans_and_all_spans_with_them():
    rng = D.Rng(9)
    src = ids("a1 b2 x y a1 b2 x y a1 b2")
    picked = total = 0
    for _ in range(800):
        got, lab = D.do_title_mask(list(src), [], TOK, rng)
        assert got == src and all(l in (-1, o) for l, o in zip(lab, src))
        picked += sum(l != -1 for l in lab)
        total += len(src)
    assert abs(picked / total - 0.15) <= _binomial_slack(total, 0.15), picked
    masked = randomised = 0
    n = 2000
    for _ in range(n):
        got, lab = D.do_title_mask(list(src), [(1, 3), (2, 4), (8, 9)], TOK, rng)
        sel = [1, 2, 3, 8]
        assert [i for i, l in enumerate(lab) if l != -1] == sel and all(lab[i] == src[i] for i in sel)      # overlapping spans too
        assert all(got[i] == src[i] for i in range(len(src)) if i not in sel)
        if [got[i] for i in sel] == [MASK] * 4:
            masked += 1
        else:
            randomised += 1
    assert abs(masked / n - 0.5) <= _binomial_slack(n, 0.5), masked


def test_property_parsing_on_edge_strings():
    t = TOK.tokenize
    assert D.process_single_property(t("颜色 红色")) == []                       # no colon
    assert D.process_single_property([]) == []
    assert D.process_single_property(t("颜色:红色;")) == [["颜色"], ["红色"]]       # trailing ';' dropped
    assert D.process_single_property(t("颜色:红色")) == [["颜色"], ["红色"]]
    assert D.process_single_property(t("颜色:;")) == [["颜色"], []]               # empty value
    assert D.process_single_property(t("颜色:")) == [["颜色"], []]
    props, spans = D.process_title_match_pvs(t("华为 手机 红色 红色"), t("颜色:红色;手机;品牌:华为;"))
    assert props == [[["颜色"], ["红色"]], [["品牌"], ["华为"]]]                   # the chunk without a colon is dropped
    assert spans == [(2, 3), (3, 4), (0, 1)]
    assert D.process_title_match_pvs(t("x y"), []) == ([], [])
    props, spans = D.process_title_match_pvs(t("华为 手机"), t("品牌:华为"))        # no trailing ';': the last chunk ends with the text
    assert props == [[["品牌"], ["华为"]]] and spans == [(0, 1)]
    props, spans = D.process_title_match_pvs(t("大号 a1"), t("尺码:大号 a1;"))      # a two-token value
    assert props == [[["尺码"], ["大号", "a1"]]] and spans == [(0, 2)]


def test_truncation_keeps_ids_and_labels_aligned():
    toks, labs = list(range(100, 120)), list(range(20))
    assert D.truncate_pairs(toks, labs, -1, D.Rng(0)) == (toks, labs)
    assert D.truncate_pairs(toks, labs, 21, D.Rng(0)) == (toks, labs)
    heads = tails = 0
    rng = D.Rng(4)
    for _ in range(200):
        a, b = D.truncate_pairs(toks, labs, 7, rng)
        assert len(a) == len(b) == 7 and [x - 100 for x in a] == b
        heads += b[0] == 0
        tails += b[-1] == 19
    assert heads + tails == 200 and heads and tails
    # through create_input_features: a property segment cut to the room left still carries each label under its own token
    seg = segments(RECORD)
    n_fixed = sum(len(s) for s in seg[:4])
    windows = [w for full in (seg[4], seg[4] + ids(";")) for w in (full[:5], full[-5:])]
    labelled = 0
    for seed in range(20):
        _, masked = D.get_masked_examples(D.record_texts(RECORD), TOK, n_fixed + 5, D.Rng(seed))
        for ex in masked:
            assert len(ex["input_ids"]) == n_fixed + 7 and ex["token_type_ids"][n_fixed + 1:n_fixed + 6] == [4] * 5
            got, lab = ex["input_ids"][n_fixed + 1:n_fixed + 6], ex["label_ids"][n_fixed + 1:n_fixed + 6]
            # one of the windows explains every position: the original token under a label, the original token where there is none
            assert any(all((l == o) if l != -1 else (g == o) for g, l, o in zip(got, lab, w)) for w in windows), (got, lab)
            labelled += any(l != -1 for l in lab)
    assert labelled


def test_the_same_seed_gives_the_same_examples(tmp_path):
    recs = [RECORD, NO_MATCH, dict(RECORD, title="x y 红色")]
    path = tmp_path / "pretrain_train.jsonl"
    path.write_text("\n".join(json.dumps(r, ensure_ascii=False) for r in recs) + "\n", encoding="utf8")

    def run(seed):
        rng = D.Rng(seed)
        out = []
        for chunk in D.read_pretrained_data(str(tmp_path), "pretrain_train.jsonl", rng, batch_size=2):
            assert len(chunk) <= 2
            out.append(D.build_examples(chunk, TOK, 50, rng))
        return out

    assert run(3) == run(3)
    assert run(3) != run(4)
    a = run(3)
    assert sum(len(b) for b in a) == 9 + 7 + 9 and all(e["next_label"] == 1 for b in a for e in b)


def test_next_examples_are_built_with_label_0_and_no_mlm_label():
    recs = [RECORD, NO_MATCH]
    out = D.get_next_examples(D.record_texts(RECORD), TOK, 50, recs, D.Rng(1), neg_sample_num=6)
    assert len(out) == 6 and all(e["next_label"] == 0 and set(e["label_ids"]) == {-1} for e in out)


def test_collate_shapes_and_dtypes():
    import torch
    ex = D.build_examples([RECORD, NO_MATCH], TOK, 50, D.Rng(2))
    got = list(D.batches(ex, 4))
    assert sum(b[0].shape[0] for b in got) == len(ex) and got[0][0].shape == (4, 52)
    ids_, mask, types, labels, nxt = got[0]
    assert mask.dtype == torch.float32 and all(t.dtype == torch.long for t in (ids_, types, labels, nxt))
    assert (mask[:, 0] == 0).all() and (labels[:, 0] == -1).all() and (nxt == 1).all()
    shuffled = list(D.batches(ex, 4, D.Rng(3)))
    assert sorted(map(tuple, torch.cat([b[0] for b in shuffled]).tolist())) == sorted(map(tuple, torch.cat([b[0] for b in got]).tolist()))
