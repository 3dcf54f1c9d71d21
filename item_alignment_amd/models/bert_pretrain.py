"""BertForPreTraining on the HIP engine: the masked-LM + next-sentence model the reference's bert_pretrain.py trains
(pytorch_transformers BertForPreTraining; reference bert_pretrain.py:508, :564-569).  The encoder is the engine's RobertaModel driven
the BERT way; the state_dict keys are transformers' (`bert.*`, `cls.predictions.*`, `cls.seq_relationship.*`), so a checkpoint written
here loads into RobertaModel / RobertaOneTower / RobertaTwoTower through PretrainedMixin.from_pretrained, which strips the `bert.` prefix.

The masked-LM head runs on the labelled rows only.  CrossEntropyLoss(ignore_index=-1) gives every other position a loss and a gradient
of exactly zero, so transform -> decoder -> loss over the M_live labelled rows is the same function as the reference's pass over all
B L rows -- with [M_live, V] logits (tens of MB) instead of [B L, V] (1.38 GB at batch 32 x 512 positions).  The three matrix
products are the engine's MFMA GEMMs; the row work over the vocabulary is csrc/vocab_ce.hip.
"""
import json
import os

import torch
from torch import nn

from .. import ops
from ..utils import ROBERTA_WEIGHTS_NAME
from . import functional as Fn
from .base import ACT_TANH, HipModule, cls_rows, init_bert_weights
from .text import PretrainedMixin, RobertaModel, adopt

BF16, F32 = torch.bfloat16, torch.float32


class BertPredictionHeadTransform(nn.Module):
    """dense -> erf-GELU -> LayerNorm (parameter holder; MaskedLMHeadFn does the arithmetic)"""

    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)


class _TiedDecoder(nn.Module):
    """`decoder.weight` of the checkpoint: the word table itself, the same Parameter"""

    def __init__(self, weight):
        super().__init__()
        self.weight = weight


class BertLMPredictionHead(nn.Module):
    def __init__(self, config, word_table):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = _TiedDecoder(word_table)
        self.bias = nn.Parameter(torch.zeros(config.vocab_size))


class BertPreTrainingHeads(nn.Module):
    def __init__(self, config, word_table):
        super().__init__()
        self.predictions = BertLMPredictionHead(config, word_table)
        self.seq_relationship = nn.Linear(config.hidden_size, 2)


def _transform_and_decode(model, x):
    """x [M, H] bf16 -> (logits [M, V] fp32, what the backward needs): dense + bias + GELU (GEMM epilogue), LayerNorm, then the decoder
    GEMM against the word table's bf16 shadow [V, H] with the bias epilogue and fp32 output"""
    A, P = model.arena, model.cls.predictions
    T = P.transform
    act, dgelu = ops.gemm(x, A.shadow_of(T.dense.weight), epilogue=ops.EPI_BIAS_GELU, bias=T.dense.bias)
    y, _, mean, rstd = ops.ln_fwd(act, T.LayerNorm.weight, T.LayerNorm.bias, T.LayerNorm.eps, write_z=False)
    logits = ops.gemm(y, A.shadow_of(P.decoder.weight), epilogue=ops.EPI_BIAS, bias=P.bias, out_f32=True)
    return logits, (act, dgelu, y, mean, rstd)


def _head_backward(model, x, saved, dlogits):
    """dlogits [M, V] bf16 -> dx [M, H] bf16; the parameter gradients are added into the arena"""
    A, P = model.arena, model.cls.predictions
    T = P.transform
    act, dgelu, y, mean, rstd = saved
    table = P.decoder.weight
    dy = ops.gemm(dlogits, A.shadow_of(table), b_kstrided=True)
    # the decoder's share of the tied word table's gradient: += into the tensor the embedding backward adds its share to
    ops.gemm(dlogits, y, a_kstrided=True, b_kstrided=True, out=table.grad, out_f32=True, accumulate=True)
    ops.colsum(dlogits, P.bias.grad, accumulate=True)
    dz, _ = ops.ln_bwd(dy, act, mean, rstd, T.LayerNorm.weight, dgamma=T.LayerNorm.weight.grad, dbeta=T.LayerNorm.bias.grad)
    # x gelu'(pre): no GEMM stands in front of this product (the LayerNorm backward does), so the IA_EPI_DGELU epilogue has nothing
    # to ride on; [M, H] elementwise, in fp32 with one bf16 rounding
    dpre = (dz.to(F32) * dgelu.to(F32)).to(BF16)
    dx = ops.gemm(dpre, A.shadow_of(T.dense.weight), b_kstrided=True)
    ops.gemm(dpre, x, a_kstrided=True, b_kstrided=True, out=T.dense.weight.grad, out_f32=True, accumulate=True)
    ops.colsum(dpre, T.dense.bias.grad, accumulate=True)
    Fn._notify([table, P.bias, T.LayerNorm.weight, T.LayerNorm.bias, T.dense.weight, T.dense.bias])
    return dx


class MaskedLMHeadFn(torch.autograd.Function):
    """BertLMPredictionHead + CrossEntropyLoss(ignore_index=-1) over the labelled rows: hidden [B L, H] bf16, rows [M] int64 (the
    labelled positions, ascending), labels [M] int64 -> the mean loss (0-d fp32)."""

    @staticmethod
    def forward(ctx, hidden, model, rows, labels):
        x = hidden.index_select(0, rows)
        logits, saved = _transform_and_decode(model, x)
        lse, _loss_row, loss = ops.vocab_ce_fwd(logits, labels)
        ctx.model, ctx.saved, ctx.shape = model, (x, rows, labels, logits, lse, loss) + saved, hidden.shape
        return loss[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        x, rows, labels, logits, lse, loss = ctx.saved[:6]
        # softmax - onehot, scaled, straight into the bf16 operand of the next two GEMMs
        dlogits = ops.vocab_ce_bwd(logits, labels, lse, loss, dloss.reshape(1).to(F32).contiguous())
        dx = _head_backward(ctx.model, x, ctx.saved[6:], dlogits)
        dh = torch.zeros(ctx.shape, device=dx.device, dtype=BF16)
        dh.index_copy_(0, rows, dx)
        ctx.saved = None
        return dh, None, None, None


class TiedCaptionHeadFn(torch.autograd.Function):
    """CoCaForPretraining's to_logits + CrossEntropyLoss(ignore_index=pad_id) over the rows whose label is not pad (reference
    multimodal.py:915-922): hidden [B n, H] bf16, rows [M] int64 (the live positions, ascending), labels [M] int64 (none of them pad)
    -> the mean loss (0-d fp32).  norm: the gamma LayerNorm (`gamma`, the zero `beta` buffer); table: the text tower's word table, whose
    bf16 shadow is the decoder's weight.  The GEMM and loss calls are MaskedLMHeadFn's, without a bias or a transform."""

    @staticmethod
    def forward(ctx, hidden, owner, norm, table, rows, labels):
        x = hidden.index_select(0, rows)
        y, _, mean, rstd = ops.ln_fwd(x, norm.gamma, norm.beta, 1e-5, write_z=False)
        logits = ops.gemm(y, owner.arena.shadow_of(table), out_f32=True)
        lse, _loss_row, loss = ops.vocab_ce_fwd(logits, labels)
        ctx.owner, ctx.norm, ctx.table, ctx.shape = owner, norm, table, hidden.shape
        ctx.saved = (x, y, mean, rstd, rows, labels, logits, lse, loss)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        x, y, mean, rstd, rows, labels, logits, lse, loss = ctx.saved
        norm, table = ctx.norm, ctx.table
        dlogits = ops.vocab_ce_bwd(logits, labels, lse, loss, dloss.reshape(1).to(F32).contiguous())
        dy = ops.gemm(dlogits, ctx.owner.arena.shadow_of(table), b_kstrided=True)
        touched = []
        if table.requires_grad:      # the decoder's share of the tied table's gradient, += beside the embedding's share
            ops.gemm(dlogits, y, a_kstrided=True, b_kstrided=True, out=table.grad, out_f32=True, accumulate=True)
            touched.append(table)
        wg = norm.gamma.requires_grad
        dx, _ = ops.ln_bwd(dy, x, mean, rstd, norm.gamma, dgamma=norm.gamma.grad if wg else None)
        if wg:
            touched.append(norm.gamma)
        Fn._notify(touched)
        dh = torch.zeros(ctx.shape, device=dx.device, dtype=BF16)
        dh.index_copy_(0, rows, dx)
        ctx.saved = None
        return dh, None, None, None, None, None


def init_the_bert_way(model):
    """What a model whose `model.bert` is a RobertaModel needs to be BERT (BertForPreTraining, BertAlignModel): the weights drawn, absolute
    positions with a trained row 0, a trainable pooler, one arena."""
    std = getattr(model.config, "initializer_range", 0.02)
    init_bert_weights(model, std)
    # BERT's position table has no padding row: position 0 is [CLS]'s, it is drawn like the others and takes its gradient
    emb = model.bert.embeddings
    emb.pos_pad = -1
    with torch.no_grad():
        nn.init.normal_(emb.position_embeddings.weight[emb.padding_idx], mean=0.0, std=std)
    for p in model.bert.pooler.parameters():      # RobertaPooler freezes itself for the pair models; the next-sentence head trains it
        p.requires_grad = True
    adopt(model, model.bert)


def save_bert_pretrained(model, save_directory):
    """pytorch_model.bin (the fp32 masters under transformers' key names) + config.json"""
    os.makedirs(save_directory, exist_ok=True)
    sd = {k: v.detach().to("cpu", F32 if v.is_floating_point() else v.dtype).clone() for k, v in model.state_dict().items()}
    torch.save(sd, os.path.join(save_directory, ROBERTA_WEIGHTS_NAME))
    cfg = model.config.to_dict() if hasattr(model.config, "to_dict") else dict(vars(model.config))
    with open(os.path.join(save_directory, "config.json"), "w", encoding="utf8") as f:
        json.dump({k: v for k, v in cfg.items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f, indent=2, sort_keys=True)


class BertForPreTraining(HipModule, PretrainedMixin):
    """model(input_ids, token_type_ids=None, attention_mask=..., masked_lm_labels=..., next_sentence_label=...) ->
    (total_loss, prediction_scores, seq_relationship_score) with both labels, (prediction_scores, seq_relationship_score) without,
    as the reference's class.  Labels use -1 for "ignore", as pytorch_transformers does.

    The one deviation: with labels, prediction_scores is None.  The reference materialises [B, L, V] fp32 logits there (1.38 GB at its
    own shape) that its training loop never reads; the loss here comes from the labelled rows alone.  Without labels the scores are
    computed densely, in fp32, by the same GEMMs."""

    def __init__(self, config):
        super().__init__()
        if config.vocab_size % 8:
            raise ValueError(f"BertForPreTraining: vocab_size {config.vocab_size} is not a multiple of 8, which the decoder GEMMs need: resize "
                             f"the word table to {(config.vocab_size + 7) // 8 * 8} rows (pad the vocabulary with unused tokens)")
        if getattr(config, "pad_token_id", 0) is None:
            config.pad_token_id = 0
        self.config = config
        self.bert = RobertaModel(config)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight)
        init_the_bert_way(self)

    def get_output_embeddings(self):
        return self.cls.predictions.decoder

    def forward(self, input_ids, token_type_ids=None, attention_mask=None, masked_lm_labels=None, next_sentence_label=None,
                position_ids=None, loss_shares=None, **unused):
        """loss_shares=(w_mlm, w_nsp): data parallelism (item_alignment_amd.dist.loss_shares) -- each of the two mean losses is scaled
        by this rank's share of the global batch's rows of its kind, so the ranks' averaged gradients are the gradient of the global
        means.  None: the model of one process.  last_losses holds the two terms as they were added."""
        self.ensure_arena()
        B, L = input_ids.shape
        dev = input_ids.device
        if position_ids is None:        # BERT's absolute positions, not RoBERTa's pad-offset ones
            position_ids = torch.arange(L, device=dev, dtype=torch.long).unsqueeze(0).expand(B, L)
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_ids)
        # allow_unpad=False: the encoder runs dense.  The reference's features give [CLS] and [SEP] attention mask 0
        # (create_input_features) and the pooler reads the [CLS] row, so a row the mask calls padded IS read here: none of the padded-row
        # shortcuts (masked_rows_dead, padded_rows_unread, IA_UNPAD) is sound for this model.
        hidden = self.bert(input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, position_ids=position_ids,
                           allow_unpad=False).last_hidden_state
        H = hidden.shape[-1]
        flat = hidden.reshape(B * L, H)
        pooled = Fn.GatherRowsFn.apply(flat, self.anchor, cls_rows(B, L, 0, dev), 0.0, 0)
        pooled = Fn.LinearSmallFn.apply(pooled, self.bert.pooler.dense.weight, self.bert.pooler.dense, ACT_TANH)
        labels = None if next_sentence_label is None else next_sentence_label.reshape(-1).to(torch.long).contiguous()
        seq_score, _probs, nsp_loss = Fn.PairHeadCEFn.apply(pooled, None, self.cls.seq_relationship, labels)
        if masked_lm_labels is None:
            with torch.no_grad():
                scores, _ = _transform_and_decode(self, flat.contiguous())
            return scores.view(B, L, -1), seq_score
        mlm = masked_lm_labels.reshape(-1).to(torch.long)
        rows = (mlm != -1).nonzero(as_tuple=False).squeeze(1)       # the one host sync of the head: M_live sizes its tensors
        if rows.numel() == 0:
            # torch's mean over no row; no kernel runs with M = 0.  Under data parallelism a weight of 0 says that another rank holds
            # labelled rows: this rank's share of the global mean is then exactly 0, not NaN
            empty = 0.0 if loss_shares is not None and float(loss_shares[0]) == 0.0 else float("nan")
            mlm_loss = torch.full((), empty, device=dev, dtype=F32)
        else:
            mlm_loss = MaskedLMHeadFn.apply(flat, self, rows, mlm.index_select(0, rows).contiguous())
        if next_sentence_label is None:
            return None, seq_score
        if loss_shares is not None:
            mlm_loss, nsp_loss = mlm_loss * float(loss_shares[0]), nsp_loss * float(loss_shares[1])
        self.last_losses = (mlm_loss.detach(), nsp_loss.detach())
        return mlm_loss + nsp_loss, None, seq_score

    def save_pretrained(self, save_directory):
        save_bert_pretrained(self, save_directory)
