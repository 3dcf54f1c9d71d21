"""Example builder of the masked-LM + next-sentence pre-training (what the reference's bert_pretrain.py does between reading a record and
handing tensors to BertForPreTraining), written from its behaviour.

A record is a JSON object with the fields FIELD_NAMES; missing ones read MISSING.  Its five texts become five segments with token
types 0..4.  From one record come several training examples, each the same sequence with one thing selected for prediction:
  * the industry name, whole (do_whole_mask);
  * the category name, whole;
  * the title: the spans that repeat a property value, or, when there is none, 15 % of its tokens (do_title_mask);
  * every property name and every property value of the property segment, one example each (do_pvs_mask).
`label_ids` is the original id at a selected position and -1 elsewhere.  A selected position keeps its token, gets a random one or
gets [MASK]; the proportions are per function, below.

Layout of one example (create_input_features): [CLS] fixed segments, property segment [SEP], then padding to max_seq_len + 2 with id 0,
attention mask 0, label -1.  [CLS] and [SEP] carry label -1 and ATTENTION MASK 0; the property segment has token type 4 and is cut to
the room left (from the front or from the back, a coin flip); `[]` when the fixed segments alone reach max_seq_len.

All randomness comes from the `Rng` pair (a numpy Generator and a random.Random) the caller hands in: a run is reproducible from one
seed.  Draw-for-draw equality with the reference's global numpy / random state is not a goal.

Kept quirk: next-sentence examples (get_next_examples: the same item with another record's properties, next_label 0) are built by the
reference and then never trained on -- its loop extends the batch with the masked examples only, so every `next_label` is 1.  The
builder is here, the loop in bert_pretrain.py leaves its output out in the same way.
"""
import json
import os
import random
from copy import deepcopy

import numpy as np
import torch

FIELD_NAMES = ["industry_name", "cate_name", "cate_name_path", "title", "item_pvs"]
MISSING = "信息缺失"
TITLE_SEGMENT, PVS_SEGMENT = 3, 4
PVS_TOKEN_TYPE = 4
IGNORE = -1


class Rng:
    """the two generators every function here draws from"""

    def __init__(self, seed):
        self.np = np.random.default_rng(seed)
        self.py = random.Random(seed)


def _token_id(tokenizer, token):
    return tokenizer.convert_tokens_to_ids([token])[0]


def read_pretrained_data(data_dir, file, rng, batch_size=1000):
    """yield the records of a JSON-lines file in shuffled chunks of batch_size (-1: the whole file as one chunk)"""
    records = []
    with open(os.path.join(data_dir, file), "r", encoding="utf8") as reader:
        for line in reader:
            line = line.strip()
            if not line:
                continue
            records.append(json.loads(line))
            if len(records) == batch_size:
                rng.py.shuffle(records)
                yield records
                records = []
    if records:
        rng.py.shuffle(records)
        yield records


def join_pretraining_data(record, field_names=FIELD_NAMES):
    return {field: record.get(field, MISSING) for field in field_names}


def record_texts(record, field_names=FIELD_NAMES):
    """the five texts of a record, '#' taken out of the property string"""
    d = join_pretraining_data(record, field_names)
    d["item_pvs"] = d["item_pvs"].replace("#", "")
    return [d[field] for field in field_names]


def truncate_pairs(tokens, label_ids, seq_len, rng):
    """ids and labels cut together to seq_len entries, from the front or from the back (a coin flip); -1 = no limit.  A sequence shorter
    than seq_len is returned as it is, without a draw."""
    if seq_len == -1 or len(tokens) < seq_len:
        return tokens, label_ids
    if rng.np.random() < 0.5:
        return tokens[:seq_len], label_ids[:seq_len]
    return tokens[-seq_len:], label_ids[-seq_len:]


def create_input_features(examples, max_seq_len, tokenizer, rng, next_label=1):
    """examples: one dict per segment (input_ids, token_type_ids, attention_mask, label_ids); the last one is the property segment."""
    input_ids, token_type_ids, attention_mask, label_ids = [], [], [], []
    for exp in examples[:-1]:
        input_ids.extend(exp["input_ids"])
        token_type_ids.extend(exp["token_type_ids"])
        attention_mask.extend(exp["attention_mask"])
        label_ids.extend(exp["label_ids"])
    fixed = len(input_ids)
    if fixed >= max_seq_len:
        return []
    pvs_ids, pvs_labels = truncate_pairs(examples[-1]["input_ids"], examples[-1]["label_ids"], max_seq_len - fixed, rng)
    input_ids = [_token_id(tokenizer, "[CLS]")] + input_ids + list(pvs_ids) + [_token_id(tokenizer, "[SEP]")]
    label_ids = [IGNORE] + label_ids + list(pvs_labels) + [IGNORE]
    token_type_ids = [0] + token_type_ids + [PVS_TOKEN_TYPE] * len(pvs_ids) + [0]
    attention_mask = [0] + attention_mask + [1] * len(pvs_ids) + [0]          # [CLS] and [SEP] are not attended
    pad = max_seq_len + 2 - len(input_ids)
    return {"input_ids": input_ids + [0] * pad, "token_type_ids": token_type_ids + [0] * pad, "attention_mask": attention_mask + [0] * pad,
            "label_ids": label_ids + [IGNORE] * pad, "next_label": next_label}


def _segments(seqs, tokenizer):
    out = []
    for idx, seq in enumerate(seqs):
        tokens = tokenizer.tokenize(seq)
        ids = tokenizer.convert_tokens_to_ids(tokens)
        out.append({"org_tokens": tokens, "input_ids": ids, "attention_mask": [1] * len(ids), "token_type_ids": [idx] * len(ids),
                    "label_ids": [IGNORE] * len(ids)})
    return out


def do_whole_mask(tokens, tokenizer, rng):
    """the whole segment is selected: 80 % it stays as it is, 10 % every token becomes a random one, 10 % every token becomes [MASK]"""
    label_ids = list(tokens)
    draw = rng.np.random()
    if draw < 0.8:
        return list(tokens), label_ids
    if draw < 0.9:
        return [int(rng.np.integers(len(tokenizer))) for _ in tokens], label_ids
    return [_token_id(tokenizer, "[MASK]")] * len(tokens), label_ids


def do_title_mask(tokens, mask_positions, tokenizer, rng):
    """mask_positions: (start, end) spans of the title that repeat a property value.  With spans: all of them are selected and, on one
    coin flip for the title, replaced by random tokens or by [MASK].  Without: every token is selected with probability 0.15 and stays
    as it is."""
    tokens = list(tokens)
    label_ids = [IGNORE] * len(tokens)
    if not mask_positions:
        for i in range(len(tokens)):
            if rng.np.random() < 0.15:
                label_ids[i] = tokens[i]
        return tokens, label_ids
    randomise = rng.np.random() < 0.5
    mask_id = _token_id(tokenizer, "[MASK]")
    for start, end in mask_positions:
        for i in range(start, min(end, len(tokens))):
            if label_ids[i] == IGNORE:               # overlapping spans: the label stays the original token
                label_ids[i] = tokens[i]
            tokens[i] = int(rng.np.integers(len(tokenizer))) if randomise else mask_id
    return tokens, label_ids


def do_pvs_mask(props, tokenizer, rng):
    """props: [name tokens, value tokens] pairs.  The property segment is rebuilt as name : value ; ...; one example per name and per value
    (in shuffled order) selects that span: 80 % it stays as it is, 10 % random tokens, 10 % [MASK]."""
    tokens, key_spans, value_spans = [], [], []
    for name, value in props:
        key_spans.append((len(tokens), len(tokens) + len(name)))
        tokens.extend(list(name) + [":"])
        value_spans.append((len(tokens), len(tokens) + len(value)))
        tokens.extend(list(value) + [";"])
    spans = value_spans + key_spans
    rng.np.shuffle(spans)
    input_ids = tokenizer.convert_tokens_to_ids(tokens)
    mask_id = _token_id(tokenizer, "[MASK]")
    examples = []
    for start, end in spans:
        ids = list(input_ids)
        label_ids = [IGNORE] * len(tokens)
        draw = rng.np.random()
        for p in range(int(start), int(end)):
            if 0.8 <= draw < 0.9:
                ids[p] = int(rng.np.integers(len(tokenizer)))
            elif draw >= 0.9:
                ids[p] = mask_id
            label_ids[p] = input_ids[p]
        examples.append({"org_tokens": tokens, "input_ids": ids, "attention_mask": [1] * len(ids), "token_type_ids": [PVS_TOKEN_TYPE] * len(ids),
                         "label_ids": label_ids})
    return examples


def process_single_property(chunk):
    """tokens of one `name : value ;` chunk -> [name tokens, value tokens]; [] without a colon.  The value may be empty."""
    if not chunk or ":" not in chunk:
        return []
    sep = chunk.index(":")
    value = chunk[sep + 1:]
    if value and value[-1] == ";":
        value = value[:-1]
    return [chunk[:sep], value]


def _match_terms(title, value):
    """(start, end) of every place where the title's tokens, joined, spell the value's.  An empty value matches everywhere with an empty
    span, as in the reference: such a title then counts as having spans and gets no label from them."""
    want = "".join(value)
    return [(i, i + len(value)) for i in range(len(title)) if "".join(title[i:i + len(value)]) == want]


def process_title_match_pvs(title, pvs):
    """title / pvs: token lists.  -> (props, the title spans that repeat a property value).  The property tokens are cut into chunks after
    every ';' (the last chunk ends with the text); chunks without a colon are dropped."""
    chunks, end = [], -1
    for idx, token in enumerate(pvs):
        if token == ";" or idx == len(pvs) - 1:
            chunks.append(pvs[end + 1:idx + 1])
            end = idx
    props = [p for p in (process_single_property(c) for c in chunks) if p]
    spans = []
    for _name, value in props:
        spans.extend(_match_terms(title, value))
    return props, spans


def process_pvs_mask(props, tokenizer, rng):
    """props: dicts with prop_name / prop_value.  Every `name:` and `value;` piece in turn is selected (its last token, the punctuation,
    excepted): 80 % as it is, 10 % [MASK], 10 % random tokens.  -> (one id sequence per piece, the label sequences).  The reference keeps
    this function without calling it; so does the loop here."""
    pieces = []
    for p in props:
        pieces.append(tokenizer.convert_tokens_to_ids(tokenizer.tokenize(p["prop_name"] + ":")))
        pieces.append(tokenizer.convert_tokens_to_ids(tokenizer.tokenize(p["prop_value"] + ";")))
    mask_id = _token_id(tokenizer, "[MASK]")
    seqs, labels = [], []
    for idx, piece in enumerate(pieces):
        body, last = piece[:-1], piece[-1:]
        draw = rng.np.random()
        if draw < 0.8:
            shown = list(piece)
        elif draw < 0.9:
            shown = [mask_id] * len(body) + last
        else:
            shown = [int(rng.np.integers(len(tokenizer))) for _ in body] + last
        left = [t for q in pieces[:idx] for t in q]
        right = [t for q in pieces[idx + 1:] for t in q]
        seqs.append(left + shown + right)
        labels.append([IGNORE] * len(left) + body + [IGNORE] * (len(last) + len(right)))
    return seqs, labels


def get_masked_examples(seqs, tokenizer, max_seq_len, rng):
    """seqs: the five texts of a record -> (the unmasked segments, the training examples)"""
    org = _segments(seqs, tokenizer)
    props, title_spans = process_title_match_pvs(org[TITLE_SEGMENT]["org_tokens"], org[PVS_SEGMENT]["org_tokens"])
    masked = []

    def emit(segment, ids, labels):
        ex = [deepcopy(e) for e in org]
        ex[segment]["input_ids"], ex[segment]["label_ids"] = ids, labels
        masked.append(create_input_features(ex, max_seq_len, tokenizer, rng))

    for segment in (0, 1):                                   # industry name, category name
        emit(segment, *do_whole_mask(org[segment]["input_ids"], tokenizer, rng))
    emit(TITLE_SEGMENT, *do_title_mask(org[TITLE_SEGMENT]["input_ids"], title_spans, tokenizer, rng))
    for feature in do_pvs_mask(props, tokenizer, rng):
        ex = [deepcopy(e) for e in org]
        ex[PVS_SEGMENT] = feature
        masked.append(create_input_features(ex, max_seq_len, tokenizer, rng))
    return org, masked


def get_next_examples(seqs, tokenizer, max_seq_len, data, rng, field_names=FIELD_NAMES, neg_sample_num=100):
    """negative next-sentence examples: the record's fixed segments with the properties of a randomly drawn record of `data`, nothing
    selected for prediction, next_label 0"""
    seqs = list(seqs)
    out = []
    for _ in range(neg_sample_num):
        other = record_texts(data[rng.py.randint(0, len(data) - 1)], field_names)
        seqs[-1] = other[-1]
        out.append(create_input_features(_segments(seqs, tokenizer), max_seq_len, tokenizer, rng, next_label=0))
    return out


def build_examples(records, tokenizer, max_seq_len, rng):
    """the reference loop's body for one chunk of records: the masked examples of every record, shuffled.  Examples that did not fit
    (create_input_features returned []) are left out -- the reference would fail on them when it stacks the tensors."""
    bunch = []
    for record in records:
        _, masked = get_masked_examples(record_texts(record), tokenizer, max_seq_len, rng)
        bunch.extend(m for m in masked if m)
    rng.py.shuffle(bunch)
    return bunch


def collate(examples):
    """-> input_ids, attention_mask (float, as the reference builds it), token_type_ids, label_ids, next_labels"""
    take = lambda key, dtype: torch.tensor([e[key] for e in examples], dtype=dtype)
    return (take("input_ids", torch.long), take("attention_mask", torch.float), take("token_type_ids", torch.long),
            take("label_ids", torch.long), take("next_label", torch.long))


def batches(examples, batch_size, rng=None):
    """collated batches of the examples in the order given, or in a random order drawn from rng (the reference's RandomSampler)"""
    order = list(range(len(examples)))
    if rng is not None:
        rng.py.shuffle(order)
    for i in range(0, len(order), batch_size):
        yield collate([examples[j] for j in order[i:i + batch_size]])
