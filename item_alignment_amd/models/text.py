"""Host-side mirror of the reference's src/models/text.py: RobertaModel, Roberta{One,Two}Tower,
PKGM{One,Two}Tower, TextCNNTwoTower — same constructor / forward signatures, outputs and state_dict keys,
encoder arithmetic on the HIP engine.  Two-tower models run both towers as ONE 2B batch (the reference runs
the same weights twice sequentially, text.py:1325-1351; the maths per sample is identical).
"""
import os

import torch
from torch import nn
import torch.nn.functional as F

from ..utils import logger, ROBERTA_WEIGHTS_NAME, KG_WEIGHTS_NAME
from . import functional as Fn
from .base import (BaseModelOutput, HipModule, RobertaClassificationHead, RobertaEmbeddings, RobertaEncoder, RobertaPKGMEmbeddings,
                   RobertaPooler, SequenceClassifierOutput, TwoTowerClassificationHead, VecSimClassificationHead, cls_rows,
                   init_bert_weights, ACT_TANH)
from .loss import make_loss, apply_loss


class PretrainedMixin:
    """`from_pretrained(path, config=cfg, ignore_mismatched_sizes=True)` of the reference classes
    (RobertaPreTrainedModel.from_pretrained; PKGM variant merges two files, reference text.py:620-654)."""

    weight_files = (ROBERTA_WEIGHTS_NAME,)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, config=None, ignore_mismatched_sizes=False, state_dict=None,
                        **kwargs):
        if config is None:
            raise ValueError("config= is required (the reference always passes a BertConfig)")
        model = cls(config, *model_args)
        merged = {}
        if state_dict is not None:
            merged.update(state_dict)
        elif pretrained_model_name_or_path is not None:
            for fn in cls.weight_files:
                f = os.path.join(str(pretrained_model_name_or_path), fn)
                if os.path.exists(f):
                    merged.update(torch.load(f, map_location="cpu"))
                else:
                    logger.warning(f"{f} not found: those weights keep their random initialisation")
        if merged:
            own = model.state_dict()
            loaded, skipped, unmatched = {}, [], []
            for k, v in merged.items():
                # checkpoint keys may carry a base-model prefix the target lacks (a bare RobertaModel as CoCa's text tower loading
                # a "roberta." / "bert." checkpoint: HF strips base_model_prefix) or lack one the target has
                bare = k.split(".", 1)[1] if k.startswith(("roberta.", "bert.")) else k
                cands = [k, "roberta." + k, k.replace("bert.", "roberta.", 1), "roberta.embeddings." + k, bare]
                tgt = next((c for c in cands if c in own), None)
                if tgt is None:
                    unmatched.append(k)
                    continue
                if own[tgt].shape != v.shape:
                    if not ignore_mismatched_sizes:
                        raise RuntimeError(f"size mismatch for {tgt}: {tuple(v.shape)} vs {tuple(own[tgt].shape)}")
                    skipped.append(tgt)
                    continue
                loaded[tgt] = v
            if not loaded:
                raise RuntimeError(f"no checkpoint key matches {cls.__name__} (first checkpoint keys: {list(merged)[:5]}, first model keys: "
                                   f"{list(own)[:5]}): the model would silently keep its random initialisation")
            model.load_state_dict(loaded, strict=False)
            if skipped:
                logger.warning(f"ignored mismatched sizes: {skipped}")
            if unmatched:
                logger.warning(f"{len(unmatched)} checkpoint keys have no counterpart in {cls.__name__} (first: {unmatched[:8]})")
            missing = [k for k in own if k not in loaded]
            if missing:
                logger.warning(f"{len(missing)} model tensors keep their random initialisation (first: {missing[:8]})")
        model.eval()
        return model


def _key_mask(attention_mask):
    return attention_mask


# IA_UNPAD=1: text towers run on the valid tokens only (RobertaModel._forward_unpadded); default off = the reference's dense padding
UNPAD = os.environ.get("IA_UNPAD", "0") == "1"


class _PaddedView:
    """hidden_states of an unpadded tower run: a tuple-like of [B, L, H] tensors built on demand from the packed [T, H] rows
    (zeros at the padding); only the layers somebody reads are scattered."""

    def __init__(self, packed, idx, B, L, cu=None):
        self.packed, self.idx, self.B, self.L, self.cu = packed, idx, B, L, cu
        self._cache = {}

    def __len__(self):
        return len(self.packed)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return tuple(self[j] for j in range(*i.indices(len(self))))
        i = i % len(self.packed)
        if i not in self._cache:
            t = self.packed[i]
            dense = torch.zeros((self.B * self.L, t.shape[-1]), device=t.device, dtype=t.dtype)
            self._cache[i] = dense.index_copy(0, self.idx, t).view(self.B, self.L, -1)
        return self._cache[i]

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class RobertaModel(HipModule, PretrainedMixin):
    """reference text.py:1084-1266."""

    def __init__(self, config, add_pooling_layer=True):
        super().__init__()
        self.config = config
        self.embeddings = RobertaEmbeddings(config)
        self.encoder = RobertaEncoder(config)
        self.pooler = RobertaPooler(config) if add_pooling_layer else None
        init_bert_weights(self, getattr(config, "initializer_range", 0.02))

    def get_input_embeddings(self):
        return self.embeddings.word_embeddings

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, cate_ids=None, head_mask=None,
                inputs_embeds=None, output_attentions=None, output_hidden_states=None, return_dict=None, allow_unpad=True,
                padded_rows_unread=False, cls_only_read=False, return_pooler_output=False, **unused):
        """return_pooler_output: the output also carries pooler_output, fp32 [B, H] = tanh(pooler.dense(h[:, 0])) (the reference returns it
        from every forward, text.py:1254; here it is two more launches -- the [CLS] gather and the small dense + tanh -- and opt-in).
        cls_only_read (with padded_rows_unread): of last_hidden_state the caller reads [:, 0] and nothing else, and reads no other hidden
        state -- the last layer then runs what follows its attention for the [CLS] rows only (RobertaEncoder.forward).  Opt-in.
        padded_rows_unread: the caller reads no hidden state of a padded position and accepts zeros there (as under IA_UNPAD): the
        forward then skips the padded rows too (IA_ROWS_DEAD_FWD of ia_layer_cfg::masked_rows_dead).  Opt-in -- a direct caller gets every position
        of last_hidden_state computed."""
        (self._root if "_root" in self.__dict__ else self).ensure_arena()
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        if return_pooler_output and self.pooler is None:
            raise ValueError("return_pooler_output=True on a model built with add_pooling_layer=False: there is no pooler to apply")
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if UNPAD and allow_unpad and cate_ids is None:
            hs = self._forward_unpadded(input_ids, attention_mask, token_type_ids, position_ids)
            if hs is not None:
                # packed rows: the [CLS] of sequence b is the first row of its run, cu_seqlens[b]
                pooled = self._pool(hs.packed[-1], hs.cu[:-1].contiguous()) if return_pooler_output else None
                return BaseModelOutput(last_hidden_state=hs[-1], pooler_output=pooled, hidden_states=hs)
        e = self.embeddings(input_ids=input_ids, position_ids=position_ids, token_type_ids=token_type_ids, cate_ids=cate_ids)
        # allow_unpad = "nothing the caller reads depends on the padded rows" (every head of the reference reads [CLS] or valid spans; the
        # cross_attn multimodal layers, which attend over ALL text positions, pass False): the padded run may then at least skip what is
        # provably zero in its backward
        dead = allow_unpad and cate_ids is None and not output_hidden_states
        hs = self.encoder(e, attention_mask, masked_rows_dead=dead, padded_rows_unread=dead and padded_rows_unread,
                          cls_only_read=dead and padded_rows_unread and cls_only_read)
        pooled = None
        if return_pooler_output:
            B, L, H = hs[-1].shape
            pooled = self._pool(hs[-1].reshape(B * L, H), cls_rows(B, L, 0, hs[-1].device))
        return BaseModelOutput(last_hidden_state=hs[-1], pooler_output=pooled, hidden_states=hs)

    def _pool(self, flat, rows):
        """tanh(pooler.dense(row)) of the given rows of a [rows, H] hidden state, fp32: the head BertAlignModel applies to its packed batch"""
        cls_h = Fn.GatherRowsFn.apply(flat, self.anchor, rows, 0.0, 0)
        return Fn.LinearSmallFn.apply(cls_h, self.pooler.dense.weight, self.pooler.dense, ACT_TANH)

    def _forward_unpadded(self, input_ids, attention_mask, token_type_ids, position_ids):
        """IA_UNPAD=1: run the tower on the valid tokens only.  The reference pads every sequence to max length and computes on the
        padding too (data.py:558-559); nothing it returns depends on those rows (keys are masked, heads read valid positions), so
        the padded rows are dropped before the embedding kernel and every layer runs on sum(lengths) rows with the packed
        attention kernels.  Hidden states come back in the padded [B, L, H] shape (zeros at the padding) on demand."""
        B, L = input_ids.shape
        ids, tts, pids = self.embeddings._ids(input_ids, token_type_ids, position_ids)
        got = self._forward_packed([(ids, tts, pids, attention_mask)], dense_is_none=True)
        if got is None:
            return None                                                                # nothing to drop
        packed, idx, cu = got
        return _PaddedView(packed, idx, B, L, cu)

    def _forward_packed(self, fields, dense_is_none=False, strict=False):
        """The tower on the valid tokens of several padded inputs at once.  fields: a list of (input_ids, token_type_ids, position_ids,
        attention_mask), each [B_f, L_f] with its own L_f.  The valid tokens of all sequences are kept back to back, field by field and
        sequence by sequence, and run as ONE ragged batch of sum(B_f) sequences: embedding + LayerNorm, then every layer with the packed
        attention kernels (ia_layer_cfg::cu_seqlens).  A padded position is never gathered, so nothing returned depends on what it holds.
        Returns (hidden states: the embedding output and every layer's, each [T, H]; idx [T]: packed row -> row of the fields' flattened
        positions laid end to end; cu_seqlens int32 [sum(B_f) + 1]).
        One host synchronisation: T sizes the tensors and the longest sequence the attention launches.
        dense_is_none: return None, with nothing launched, when no position is padded.
        strict: a sequence without a valid token, or whose position 0 is not one, raises ValueError with nothing launched."""
        emb, enc = self.embeddings, self.encoder
        dev = fields[0][0].device
        valid = [(f[3] != 0) for f in fields]
        lens = torch.cat([v.sum(dim=1) for v in valid])
        first = torch.cat([v[:, 0] for v in valid]).all().to(lens.dtype)
        T, Lmax, Lmin, first = (int(v) for v in torch.stack((lens.sum(), lens.max(), lens.min(), first)).tolist())   # the one host sync
        S = lens.numel()
        if strict and Lmin == 0:
            raise ValueError("a sequence has an attention mask of zeros only: there is no token to run (the padded form would attend "
                             "uniformly over its padding)")
        if strict and not first:
            raise ValueError("a sequence's position 0 is masked: the packed run reads the first valid token of each sequence as its [CLS]")
        flat_valid = torch.cat([v.reshape(-1) for v in valid])
        N = flat_valid.numel()
        if dense_is_none and T == N:
            return None
        # packed row -> flattened position, without a second synchronisation (nonzero() would be one): every valid position writes its
        # own number into the slot its running count names, every padded one into a spare slot behind the end
        slot = torch.cumsum(flat_valid, 0) - 1
        idx = torch.empty(T + 1, device=dev, dtype=torch.long)
        idx.scatter_(0, torch.where(flat_valid, slot, torch.full_like(slot, T)), torch.arange(N, device=dev, dtype=torch.long))
        idx = idx[:T]
        cu = torch.zeros(S + 1, device=dev, dtype=torch.int32)
        cu[1:] = torch.cumsum(lens, 0)
        training = self.training and torch.is_grad_enabled()
        p = emb.drop_p if training else 0.0
        take = lambda k: torch.cat([f[k].reshape(-1) for f in fields]).index_select(0, idx).contiguous()
        pk = take(2)
        order = torch.argsort(pk, stable=True).to(torch.int32)          # backward walks the rows position by position (embed.hip)
        e = Fn.EmbedLNFn.apply(emb.anchor, emb, take(0), take(1), pk, None, None, p, emb.stream_id, order)
        outs = Fn.EncoderStackFn.apply(e, enc.anchor, enc, None, S, Lmax, torch.is_grad_enabled(), cu, Fn.StackRows())     # no masked row
        return (e,) + tuple(outs), idx, cu


def adopt(root, *children):
    """sub-models built on their own (CoCa passes ready-made encoders in) share the root's arena."""
    for c in children:
        for m in c.modules():
            m.__dict__["_root"] = root


class _PairTowerBase(HipModule, PretrainedMixin):
    def _finish(self, logits, probs, loss, src, tgt, labels, hidden_states=None):
        cfg = self.config
        if labels is not None and cfg.loss_type != "ce":
            loss = apply_loss(self.loss_fct, cfg, logits, labels, src, tgt)
        return SequenceClassifierOutput(loss=loss, logits=logits, probs=probs, src_embeds=src, tgt_embeds=tgt, hidden_states=hidden_states)


class AuxiliaryTaskPair(nn.Module):
    """reference text.py:66-102: for every (source attribute, target attribute) pair with the same key, the mean token vector of
    each `key:value` span -> dropout -> Linear(2H -> num_labels); labels say whether the values are equal.  `pair_indices` is
    the per-sample list the dataset builds (data.py:568-612): rows of (src start, src end, tgt start, tgt end, label).
    Returns the mean cross-entropy over all pairs of the batch (what `self.loss_fct(logits2, labels2)` adds at :1478-1480)."""

    def __init__(self, config):
        super().__init__()
        drop = getattr(config, "classifier_dropout", None)
        self.drop_p = float(drop if drop is not None else config.hidden_dropout_prob)
        self.out_proj = nn.Linear(config.hidden_size * 2, config.num_labels)

    def forward(self, taps, pair_indices, anchor, B, L, training):
        import numpy as np
        rows, ptr_, labels = [], [0], []
        for i, pi in enumerate(pair_indices):
            pi = pi.detach().cpu().numpy() if torch.is_tensor(pi) else np.asarray(pi)
            for j in range(pi.shape[0] if pi.ndim == 2 else 0):
                a0, a1, b0, b1, lab = (int(v) for v in pi[j])
                rows += [(i * L + a0, i * L + a1), (i * L + b0, i * L + b1)]
                labels.append(lab)
            ptr_.append(len(rows))
        ptr_ += [len(rows)] * (B + 1 - len(ptr_))
        if not labels:
            raise RuntimeError("auxiliary_task: no attribute pairs in this batch (the reference's torch.stack of an empty list fails likewise)")
        dev = taps[0].device
        spans = torch.tensor(rows, dtype=torch.int32, device=dev)
        span_ptr = torch.tensor(ptr_, dtype=torch.int32, device=dev)
        labels2 = torch.tensor(labels, dtype=torch.int64, device=dev)
        H = taps[0].shape[-1]
        means = [Fn.SpanMeanFn.apply(t.reshape(B * L, H), anchor, spans, span_ptr, B, L) for t in taps]
        m = means[0] if len(means) == 1 else torch.stack(means).mean(dim=0)
        x, y = m[0::2], m[1::2]
        if training and self.drop_p > 0:
            x, y = F.dropout(x, self.drop_p, True), F.dropout(y, self.drop_p, True)
        _logits, _probs, loss = Fn.PairHeadCEFn.apply(x, y, self.out_proj, labels2)
        return loss


class RobertaOneTower(_PairTowerBase):
    """reference text.py:1379-1492."""
    supports_auxiliary = True          # only this class builds AuxiliaryTaskPair in the reference (text.py:1412-1413)

    def __init__(self, config):
        super().__init__()
        self.num_labels = config.num_labels
        self.config = config
        if config.max_seq_len_pv is None:
            self.max_seq_len = config.max_seq_len
        elif config.max_seq_len is None:
            self.max_seq_len = config.max_seq_len_pv
        else:
            self.max_seq_len = config.max_seq_len + config.max_seq_len_pv
        self.cls_layers = [-int(i) for i in config.cls_layers.split(",")]
        self.roberta = self._make_backbone(config)
        if config.classification_method == "vec_sim":
            self.classifier = VecSimClassificationHead(config)
        else:
            self.classifier = RobertaClassificationHead(config)
        self.loss_fct = make_loss(config)
        if getattr(config, "auxiliary_task", False) and type(self).supports_auxiliary:
            self._build_auxiliary(config)
        init_bert_weights(self, getattr(config, "initializer_range", 0.02))
        adopt(self, self.roberta)

    def _build_auxiliary(self, config):
        if config.cls_pool != "avg" and len(self.cls_layers) > 1:
            raise ValueError("auxiliary_task needs a hidden_size-wide sequence output: one cls layer or cls_pool='avg' "
                             "(reference text.py:77: out_proj is Linear(2 * hidden_size, num_labels))")
        self.auxiliary_task = AuxiliaryTaskPair(config)

    def _make_backbone(self, config):
        return RobertaModel(config, add_pooling_layer=False)

    def _backbone(self, input_ids, attention_mask, token_type_ids, position_ids, cate_ids, inputs_embeds, image_indices,
                  hidden_states_asked=False):
        # the auxiliary attribute-pair task averages hidden states over caller-given spans (reference text.py:66-102), which may reach
        # into padded positions (the reference computes those rows like any other; the golden fixture's third sample does exactly that):
        # with it, the padded rows matter -- no unpadded run, no skipped query blocks in the attention backward
        # ... and so they do under vec_sim: the target embedding is read at the FIXED position max_seq_len (reference text.py:1463), which is a
        # padded position whenever a sequence is shorter than that (the eight-sample golden fixtures hold two such sequences: the row-wise
        # LayerNorm filter of round 6 caught it -- the 32-position attention blocks had not)
        rows_matter = hasattr(self, "auxiliary_task") or self.config.classification_method == "vec_sim"
        # (a caller that asked for the hidden states gets every position of them computed: the forward keeps the padded rows)
        return self.roberta(input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, position_ids=position_ids,
                            cate_ids=cate_ids, allow_unpad=not rows_matter,
                            padded_rows_unread=not rows_matter and not hidden_states_asked)

    def _tgt_index(self):
        return self.max_seq_len

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, cate_ids=None, head_mask=None,
                inputs_embeds=None, image_indices=None, labels=None, output_attentions=None, output_hidden_states=None,
                return_dict=None):
        self.ensure_arena()
        outputs = self._backbone(input_ids, attention_mask, token_type_ids, position_ids, cate_ids, inputs_embeds, image_indices,
                                 hidden_states_asked=bool(output_hidden_states))
        hs = outputs.hidden_states
        B, L, H = hs[-1].shape
        dev = hs[-1].device
        training = self.training and torch.is_grad_enabled()
        p = self.classifier.drop_p if training else 0.0
        taps = [hs[i] for i in self.cls_layers]

        def pick(index, sid):
            rows = cls_rows(B, L, index, dev)
            feats = [Fn.GatherRowsFn.apply(t.reshape(B * L, H), self.anchor, rows, 0.0, 0) for t in taps]
            f = torch.stack(feats).mean(dim=0) if self.config.cls_pool == "avg" else torch.cat(feats, dim=-1)
            if p > 0:
                f = F.dropout(f, p, True)
            return f

        if self.config.classification_method == "vec_sim":
            src, tgt, logits, probs = self.classifier(pick(0, 0), pick(self._tgt_index(), 1))
            loss = None
        else:
            ce = self.config.loss_type == "ce"
            logits, probs2, loss = self.classifier(pick(0, 0), labels if ce else None, inputs_embeds=inputs_embeds,
                                                   differentiable_logits=(labels is not None and not ce))
            src, tgt, probs = probs2[:, 0], probs2[:, 1], probs2[:, 1]
        out = self._finish(logits, probs, loss, src, tgt, labels, hidden_states=hs if output_hidden_states else None)
        if labels is not None and hasattr(self, "auxiliary_task"):
            if self.config.loss_type != "ce":
                raise ValueError("auxiliary_task adds self.loss_fct(logits2 [P, 2], labels2 [P]) (reference text.py:1478-1480): only "
                                 "--loss_type ce has that signature")
            out.loss = out.loss + self.auxiliary_task(taps, image_indices, self.anchor, B, L, training)
        return out


class RobertaTwoTower(_PairTowerBase):
    """reference text.py:1269-1376 (probs stay [B, 2], embeddings are the dropped-out CLS vectors: quirk A3)."""

    def __init__(self, config):
        super().__init__()
        self.num_labels = config.num_labels
        self.config = config
        self.roberta = self._make_backbone(config)
        self.classifier = TwoTowerClassificationHead(config.hidden_size, dropout=config.hidden_dropout_prob, num_labels=config.num_labels)
        self.loss_fct = make_loss(config)
        init_bert_weights(self, getattr(config, "initializer_range", 0.02))
        adopt(self, self.roberta)

    def _make_backbone(self, config):
        return RobertaModel(config, add_pooling_layer=False)

    def _both(self, a, b):
        if a is None or b is None:
            return None
        return torch.cat((a, b), dim=0)

    def _backbone(self, ids, mask, tts, pids, extra1=None, extra2=None):
        # the head reads the two [CLS] rows only and the wrapper returns no hidden states: the padded rows are neither differentiated
        # nor computed
        return self.roberta(ids, attention_mask=mask, token_type_ids=tts, position_ids=pids, padded_rows_unread=True).last_hidden_state

    def forward(self, input_ids_1=None, attention_mask_1=None, token_type_ids_1=None, cate_ids_1=None, position_ids_1=None,
                input_ids_2=None, attention_mask_2=None, token_type_ids_2=None, cate_ids_2=None, position_ids_2=None,
                head_mask=None, inputs_embeds=None, labels=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                images_1=None, images_2=None):
        self.ensure_arena()
        if input_ids_1.shape != input_ids_2.shape:
            raise ValueError("both towers must be padded to the same length (the reference collate pads to max_length)")
        if attention_mask_1 is None:
            attention_mask_1 = torch.ones_like(input_ids_1)
        if attention_mask_2 is None:
            attention_mask_2 = torch.ones_like(input_ids_2)
        B, L = input_ids_1.shape
        seq = self._backbone(self._both(input_ids_1, input_ids_2), self._both(attention_mask_1, attention_mask_2),
                             self._both(token_type_ids_1, token_type_ids_2), self._both(position_ids_1, position_ids_2), images_1, images_2)
        L, H = seq.shape[1], seq.shape[-1]          # PKGM sequences grow after embedding (each relation -> 2 rows)
        dev = seq.device
        training = self.training and torch.is_grad_enabled()
        p = self.classifier.drop_p if training else 0.0
        flat = seq.reshape(2 * B * L, H)
        f1 = Fn.GatherRowsFn.apply(flat, self.anchor, cls_rows(B, L, 0, dev), p, 2001)
        f2 = Fn.GatherRowsFn.apply(flat, self.anchor, (cls_rows(B, L, 0, dev) + B * L).contiguous(), p, 2002)
        ce = self.config.loss_type == "ce"
        src, tgt, logits, probs, loss = self.classifier(f1, f2, labels if ce else None, differentiable_logits=(labels is not None and not ce))
        return self._finish(logits, probs, loss, src, tgt, labels)


# ------------------------------------------------------------------------------------------------ PKGM
class RobertaPKGMModel(HipModule, PretrainedMixin):
    """reference text.py:128-289."""
    weight_files = (ROBERTA_WEIGHTS_NAME, KG_WEIGHTS_NAME)

    def __init__(self, config, add_pooling_layer=False):
        super().__init__()
        self.config = config
        self.embeddings = RobertaPKGMEmbeddings(config)
        self.encoder = RobertaEncoder(config)
        self.pooler = None
        init_bert_weights(self, getattr(config, "initializer_range", 0.02))

    def forward(self, input_ids, attention_mask, token_type_ids, position_ids, inputs_embeds=None, head_mask=None, masked_rows_dead=False,
                **unused):
        """masked_rows_dead: the caller reads no hidden state of a masked position (RobertaEncoder.forward)"""
        (self._root if "_root" in self.__dict__ else self).ensure_arena()
        if input_ids is None or attention_mask is None or token_type_ids is None or position_ids is None:
            raise ValueError("You have to specify input_ids, attention_mask, token_type_ids and position_ids")
        e = self.embeddings(input_ids=input_ids, position_ids=position_ids, token_type_ids=token_type_ids)
        hs = self.encoder(e, attention_mask, masked_rows_dead=masked_rows_dead)
        return BaseModelOutput(last_hidden_state=hs[-1], hidden_states=hs)


class PKGMOneTower(RobertaOneTower):
    """reference text.py:691-783 (+ two-file from_pretrained :785-1080)."""
    supports_auxiliary = False
    weight_files = (ROBERTA_WEIGHTS_NAME, KG_WEIGHTS_NAME)

    def __init__(self, config):
        if not hasattr(config, "cls_layers"):
            config.cls_layers, config.cls_pool = "1", "cat"
        if getattr(config, "max_seq_len_pv", None) is None and not hasattr(config, "max_seq_len_pv"):
            config.max_seq_len_pv = None
        super().__init__(config)
        self.cls_layers = [-1]                      # PKGMOneTower always classifies on the last layer (text.py:753-760)

    def _make_backbone(self, config):
        return RobertaPKGMModel(config, add_pooling_layer=False)

    def _backbone(self, input_ids, attention_mask, token_type_ids, position_ids, cate_ids, inputs_embeds, image_indices,
                  hidden_states_asked=False):
        # the cls head reads position 0 of the last layer only; vec_sim reads a fixed second position (RobertaOneTower._backbone)
        return self.roberta(input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, position_ids=position_ids,
                            masked_rows_dead=self.config.classification_method != "vec_sim")

    def _tgt_index(self):
        return self.config.max_seq_len + 2 * self.config.max_pvs


class PKGMTwoTower(RobertaTwoTower):
    """reference text.py:292-391."""
    weight_files = (ROBERTA_WEIGHTS_NAME, KG_WEIGHTS_NAME)

    def _make_backbone(self, config):
        return RobertaPKGMModel(config, add_pooling_layer=False)


# --------------------------------------------------------------------------------------------- TextCNN
class _CpuEmbeddings(nn.Module):
    """RobertaEmbeddings of the TextCNN model (BASELINE.json configs[0]) as plain torch modules: what runs when the input is on the
    CPU.  With the input on the GPU the same parameters are read by ia_embed_ln_fwd / _bwd (TextCNN._features_hip) and this
    forward is not called."""

    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, padding_idx=config.pad_token_id)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)
        self.register_buffer("position_ids", torch.arange(config.max_position_embeddings).expand((1, -1)))
        self.padding_idx = config.pad_token_id
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size, padding_idx=self.padding_idx)

    def forward(self, input_ids):
        from .base import create_position_ids_from_input_ids
        pos = create_position_ids_from_input_ids(input_ids, self.padding_idx)
        e = self.word_embeddings(input_ids) + self.token_type_embeddings(torch.zeros_like(input_ids))
        e = e + self.position_embeddings(pos)
        return self.dropout(self.LayerNorm(e))


class TextCNN(nn.Module):
    """reference text.py:1496-1527.  Input on the CPU: plain torch, as the reference.  Input on the GPU: Fn.TextCNNTowerFn (embedding
    gather + LayerNorm kernels, the tap projection through the bf16 GEMM, csrc/textcnn.hip for relu + max over time and its
    backward); the parameters stay ordinary nn.Parameters outside any arena."""

    def __init__(self, config, embedding_state_dict):
        super().__init__()
        filter_sizes = [int(i) for i in config.filter_sizes.split(",")]
        self.filter_sizes = filter_sizes
        self._taps, self._taps_key = None, None
        self.embedding1 = _CpuEmbeddings(config)
        self.embedding1.load_state_dict(embedding_state_dict, strict=False)
        self.embedding2 = _CpuEmbeddings(config)
        self.embedding2.load_state_dict(embedding_state_dict, strict=False)
        for value in self.embedding2.parameters():
            value.requires_grad = False
        self.convs1 = nn.ModuleList([nn.Conv2d(2, config.num_filters, (K, config.hidden_size)) for K in filter_sizes])
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, x):
        if x.is_cuda:
            return self._features_hip(x, 0.0, 3001)
        x = torch.stack((self.embedding1(x), self.embedding2(x)), dim=1)
        x = [F.relu(conv(x)).squeeze(3) for conv in self.convs1]
        x = [F.max_pool1d(i, i.size(2)).squeeze(2) for i in x]
        return self.dropout(torch.cat(x, 1))

    def tap_shadow(self):
        """bf16 [2, NTP, H] copy of the conv weights in tap order (include/itemalign.h), repacked whenever a weight has been written
        since the last pack -- after every optimiser step while training, once for an evaluation."""
        from .. import ops
        ws = [c.weight for c in self.convs1]
        key = tuple((w.data_ptr(), w._version) for w in ws)
        if key != self._taps_key:
            with torch.no_grad():
                reuse = self._taps if (self._taps is not None and self._taps.device == ws[0].device) else None
                self._taps = ops.textcnn_pack_taps([w.detach() for w in ws], self.filter_sizes, reuse)
            self._taps_key = key
        return self._taps

    def _features_hip(self, ids, p_head, stream_base):
        """dropout_head(dropout(features)) on the GPU: both dropouts are drawn inside ia_textcnn_pool_fwd (p_head = 0: the first only).
        As with nn.Dropout on the CPU path, the rates follow self.training alone; torch.no_grad only decides what is kept."""
        training = self.training
        e1 = self.embedding1
        params = [e1.word_embeddings.weight, e1.token_type_embeddings.weight, e1.position_embeddings.weight, e1.LayerNorm.weight,
                  e1.LayerNorm.bias] + [c.weight for c in self.convs1] + [c.bias for c in self.convs1]
        return Fn.TextCNNTowerFn.apply(ids, self, self.tap_shadow(), e1.dropout.p if training else 0.0, self.dropout.p if training else 0.0,
                                       p_head if training else 0.0, stream_base, torch.is_grad_enabled(), *params)


class _TorchTwoTowerHead(nn.Module):
    def __init__(self, hidden_size, dropout=0.0, num_labels=2):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.out_proj = nn.Linear(hidden_size * 2, num_labels)

    def forward(self, a, b):
        x, y = self.dropout(a), self.dropout(b)
        logits = self.out_proj(torch.cat((x, y), dim=1))
        return x, y, logits, torch.softmax(logits, dim=1)


class TextCNNTwoTower(nn.Module):
    """reference text.py:1530-1609 — BASELINE.json configs[0], the reference's CPU-runnable plumbing case."""

    def __init__(self, config, embedding_state_dict):
        super().__init__()
        self.num_labels = config.num_labels
        self.config = config
        self.textcnn = TextCNN(config, embedding_state_dict)
        if config.classification_method == "vec_sim":
            raise NotImplementedError("TextCNN + vec_sim is not used by the reference scripts (finetune_text.py never sets similarity_measure, quirk A14)")
        hidden_size = len(config.filter_sizes.split(",")) * config.num_filters
        self.classifier = _TorchTwoTowerHead(hidden_size, config.hidden_dropout_prob)
        self.loss_fct = make_loss(config)

    def forward(self, input_ids_1=None, attention_mask_1=None, token_type_ids_1=None, position_ids_1=None, input_ids_2=None,
                attention_mask_2=None, token_type_ids_2=None, position_ids_2=None, head_mask=None, inputs_embeds=None, labels=None,
                output_attentions=None, output_hidden_states=None, return_dict=None):
        if input_ids_1.is_cuda:
            return self._forward_hip(input_ids_1, input_ids_2, labels)
        o1, o2 = self.textcnn(input_ids_1), self.textcnn(input_ids_2)
        src, tgt, logits, probs = self.classifier(o1, o2)
        src, tgt, probs = probs[:, 0], probs[:, 1], probs[:, 1]
        loss = apply_loss(self.loss_fct, self.config, logits, labels, src, tgt, ce_too=True) if labels is not None else None
        return SequenceClassifierOutput(loss=loss, probs=probs, logits=logits, src_embeds=src, tgt_embeds=tgt)

    def _forward_hip(self, ids1, ids2, labels):
        """The same forward with the input on the GPU: one Fn.TextCNNTowerFn per tower (the head's dropout is drawn in its pool kernel),
        then the fused pair head + cross-entropy; the other loss types take the [B, 2] logits as on the CPU."""
        head = self.classifier
        o1 = self.textcnn._features_hip(ids1, head.dropout.p, 3001)
        o2 = self.textcnn._features_hip(ids2, head.dropout.p, 3011)
        w, b = head.out_proj.weight, head.out_proj.bias
        if labels is None or self.config.loss_type == "ce":
            logits, probs2, loss = Fn.PairHeadCEParamFn.apply(o1, o2, w, b, None if labels is None else labels.contiguous())
            if labels is None:
                loss = None
        else:
            logits = F.linear(torch.cat((o1, o2), dim=1), w, b)
            probs2 = torch.softmax(logits, dim=1)
            loss = apply_loss(self.loss_fct, self.config, logits, labels, probs2[:, 0], probs2[:, 1], ce_too=True)
        return SequenceClassifierOutput(loss=loss, probs=probs2[:, 1], logits=logits, src_embeds=probs2[:, 0], tgt_embeds=probs2[:, 1])
