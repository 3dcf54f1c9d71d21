"""Host-side mirror of the reference's src/models/multimodal.py: RobertaImage{Model,OneTower,TwoTower}
(RoBERTa + pre-extracted image embeddings), CoCaForItemAlignment (RoBERTa text tower + ViT image tower) and CoCaForPretraining
(the same towers under causal multimodal layers, trained with a caption loss and a contrastive loss).
"""
import os

import torch
from torch import nn

from . import functional as Fn
from .bert_pretrain import TiedCaptionHeadFn, _TiedDecoder
from .base import (ACT_NONE, BaseModelOutput, HipModule, RobertaEmbeddings, RobertaEncoder, RobertaImageEmbeddings, RobertaPooler,
                   SequenceClassifierOutput, TwoTowerClassificationHead, VecSimClassificationHead, cls_rows, init_bert_weights)
from .image import VisionTransformer
from .loss import apply_loss, make_loss
from .text import PretrainedMixin, RobertaOneTower, RobertaTwoTower, adopt


TOWER_STREAMS = os.environ.get("IA_TOWER_STREAMS", "0") == "1"      # module switch (bench.py flips it for its variant line)


class RobertaImageModel(HipModule, PretrainedMixin):
    """reference multimodal.py:23-210."""

    def __init__(self, config, add_pooling_layer=True):
        super().__init__()
        self.config = config
        self.embeddings = RobertaImageEmbeddings(config) if config.ensemble == "begin" else RobertaEmbeddings(config)
        self.encoder = RobertaEncoder(config)
        self.pooler = RobertaPooler(config) if add_pooling_layer else None
        init_bert_weights(self, getattr(config, "initializer_range", 0.02))

    def forward(self, input_ids=None, attention_mask=None, token_type_ids=None, position_ids=None, head_mask=None, inputs_embeds=None,
                image_indices=None, **unused):
        (self._root if "_root" in self.__dict__ else self).ensure_arena()
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids)
        if self.config.ensemble == "begin":
            e = self.embeddings(input_ids=input_ids, position_ids=position_ids, token_type_ids=token_type_ids, inputs_embeds=inputs_embeds,
                                attention_mask=attention_mask, image_indices=image_indices)
        else:
            e = self.embeddings(input_ids=input_ids, position_ids=position_ids, token_type_ids=token_type_ids)
        hs = self.encoder(e, attention_mask)
        return BaseModelOutput(last_hidden_state=hs[-1], hidden_states=hs)


class RobertaImageOneTower(RobertaOneTower):
    """reference multimodal.py:213-320."""
    supports_auxiliary = False

    def _make_backbone(self, config):
        return RobertaImageModel(config, add_pooling_layer=False)

    def _backbone(self, input_ids, attention_mask, token_type_ids, position_ids, cate_ids, inputs_embeds, image_indices,
                  hidden_states_asked=False):
        return self.roberta(input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, position_ids=position_ids,
                            inputs_embeds=inputs_embeds, image_indices=image_indices)


class RobertaImageTwoTower(RobertaTwoTower):
    """reference multimodal.py:323-461 (keyword order: ..., position_ids_1, images_1, ..., images_2, head_mask, labels)."""

    def _make_backbone(self, config):
        return RobertaImageModel(config, add_pooling_layer=False)

    def _backbone(self, ids, mask, tts, pids, images_1=None, images_2=None):
        imgs = torch.cat((images_1, images_2), dim=0) if images_1 is not None else None
        return self.roberta(ids, attention_mask=mask, token_type_ids=tts, position_ids=pids, inputs_embeds=imgs).last_hidden_state

    def forward(self, input_ids_1=None, attention_mask_1=None, token_type_ids_1=None, position_ids_1=None, images_1=None,
                input_ids_2=None, attention_mask_2=None, token_type_ids_2=None, position_ids_2=None, images_2=None, head_mask=None,
                labels=None, output_attentions=None, output_hidden_states=None, return_dict=None):
        return super().forward(input_ids_1=input_ids_1, attention_mask_1=attention_mask_1, token_type_ids_1=token_type_ids_1,
                               position_ids_1=position_ids_1, input_ids_2=input_ids_2, attention_mask_2=attention_mask_2,
                               token_type_ids_2=token_type_ids_2, position_ids_2=position_ids_2, labels=labels, images_1=images_1,
                               images_2=images_2)


class CoCaModel(nn.Module):
    """reference multimodal.py:709-840: holder of the two encoders (state_dict prefix coca.{img,text}_encoder)."""

    def __init__(self, config, image_encoder=None, text_encoder=None):
        super().__init__()
        self.config = config
        self.img_encoder = image_encoder
        self.text_encoder = text_encoder

    def embed_text(self, input_ids, attention_mask, token_type_ids, position_ids, padded_rows_matter=False, cls_only_read=False):
        # padded_rows_matter: the caller reads the hidden states of PADDED positions (the cross_attn multimodal layers attend
        # over all L text tokens without a padding mask, reference multimodal.py:529-616), so the unpadded tower run (IA_UNPAD),
        # which leaves zeros there, must not be used
        out = self.text_encoder(input_ids, attention_mask=attention_mask, token_type_ids=token_type_ids, position_ids=position_ids,
                                allow_unpad=not padded_rows_matter, padded_rows_unread=not padded_rows_matter,
                                cls_only_read=cls_only_read and not padded_rows_matter)
        return out.last_hidden_state

    def embed_image(self, images, cls_only=False):
        # cls_only: the caller reads token 0 of every image and nothing else (VisionTransformer.forward_features)
        if cls_only and isinstance(self.img_encoder, VisionTransformer):
            return self.img_encoder.forward_features(images, cls_only=True)
        return self.img_encoder.forward_features(images)


class LayerNorm(nn.Module):
    """reference multimodal.py:475-482: LayerNorm with a learned gamma and a constant zero `beta` buffer."""

    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))
        self.register_buffer("beta", torch.zeros(dim))

    def forward(self, x2d):
        return Fn.GammaLayerNormFn.apply(x2d, self.gamma, self.beta, 1e-5)


class RotaryEmbedding(nn.Module):
    """reference multimodal.py:495-506.  Only the `inv_freq` buffer lives here (state_dict parity); the rotation itself
    is computed inside ia_rotary_split_fwd from the same closed form."""

    def __init__(self, dim):
        super().__init__()
        self.register_buffer("inv_freq", 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim)))


class SwiGLU(nn.Module):
    """reference multimodal.py:521-524 (parameter-free; keeps the Sequential indices `ff_out.1` / `ff.0`, `ff.2`)."""

    def forward(self, x2d):
        return Fn.SwiGLUFn.apply(x2d)


class Residual(nn.Module):
    """reference multimodal.py:486-492.  The `+ x` is folded into the wrapped block's last GEMM epilogue."""

    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x2d, *args, **kwargs):
        return self.fn(x2d, *args, residual=x2d, **kwargs)


def _check_head_dim(dim_head):
    if dim_head != 64:
        raise NotImplementedError(f"the fused attention kernels are built for head dim 64 (got {dim_head}); "
                                  "coca_base (768/12) and coca_large (1024/16) both give 64")


class ParallelTransformerBlock(nn.Module):
    """reference multimodal.py:529-626 (no `attn_mask` argument -- nothing in the reference passes one):
    LN -> one fused projection -> multi-query attention with rotary q/k  ||  SwiGLU feed-forward -> attn_out + ff_out.
    is_decoding=True (the decoder layers of CoCa pre-training) puts the reference's triu mask on the attention: token i attends
    tokens j <= i.  The reference's `mask` and `pos_emb` buffers are non-persistent caches, so there is nothing to keep here:
    state-dict keys are the same either way."""

    def __init__(self, dim, dim_head=64, heads=8, ff_mult=4, is_decoding=False):
        super().__init__()
        _check_head_dim(dim_head)
        self.is_decoding = bool(is_decoding)
        self.norm = LayerNorm(dim)
        attn_inner_dim, ff_inner_dim = dim_head * heads, dim * ff_mult
        self.fused_dims = (attn_inner_dim, dim_head, dim_head, ff_inner_dim * 2)
        self.heads, self.scale, self.ff_inner_dim = heads, dim_head ** -0.5, ff_inner_dim
        self.rotary_emb = RotaryEmbedding(dim_head)
        self.fused_attn_ff_proj = nn.Linear(dim, sum(self.fused_dims), bias=False)
        self.attn_out = nn.Linear(attn_inner_dim, dim, bias=False)
        self.ff_out = nn.Sequential(SwiGLU(), nn.Linear(ff_inner_dim, dim, bias=False))

    def forward(self, x2d, B, n, residual=None):
        h = self.heads
        xn = self.norm(x2d)
        fused = Fn.LinearBf16Fn.apply(xn, None, self.fused_attn_ff_proj.weight, self)
        q, kv, s = Fn.FusedSplitFn.apply(fused, n, h, self.ff_inner_dim)
        # multi-query attention: every query head attends to the single k/v head -> fold the heads into query rows
        if self.is_decoding:      # folded row r is head r % h of token r // h: it attends keys j <= r // h
            o = Fn.AttentionCausalXFn.apply(q.view(B * n * h, 64), kv, B, 1, n, h, self.scale)
        else:
            o = Fn.AttentionXFn.apply(q.view(B * n * h, 64), kv, B, 1, n * h, n, self.scale)
        y = Fn.LinearBf16Fn.apply(o.view(B * n, h * 64), residual, self.attn_out.weight, self)
        # (s is not kept for ff_out's weight gradient: backward recomputes it from the x | gate columns of `fused`, which FusedSplitFn holds)
        return Fn.LinearBf16Fn.apply(s, y, self.ff_out[1].weight, self, (fused, h * 64 + 128, self.ff_inner_dim))


class CrossAttention(nn.Module):
    """reference multimodal.py:630-706 (parallel_ff=True, norm_context=False as CoCaForItemAlignment builds it, :957-960):
    queries from the text tokens, one key/value head from the image tokens, plus a parallel SwiGLU feed-forward."""

    def __init__(self, dim, *, context_dim=None, dim_head=64, heads=8, parallel_ff=False, ff_mult=4, norm_context=False):
        super().__init__()
        _check_head_dim(dim_head)
        self.heads, self.scale = heads, dim_head ** -0.5
        inner_dim = heads * dim_head
        context_dim = dim if context_dim is None else context_dim
        self.context_dim = context_dim
        self.norm = LayerNorm(dim)
        self.context_norm = LayerNorm(context_dim) if norm_context else nn.Identity()
        self.to_q = nn.Linear(dim, inner_dim, bias=False)
        self.to_kv = nn.Linear(context_dim, dim_head * 2, bias=False)
        self.to_out = nn.Linear(inner_dim, dim, bias=False)
        ff_inner_dim = ff_mult * dim
        self.ff = nn.Sequential(nn.Linear(dim, ff_inner_dim * 2, bias=False), SwiGLU(), nn.Linear(ff_inner_dim, dim, bias=False)) \
            if parallel_ff else None

    def forward(self, x2d, ctx2d, B, n, n_ctx, residual=None):
        h = self.heads
        if ctx2d.shape[-1] != self.context_dim:
            raise ValueError(f"CrossAttention: context width {ctx2d.shape[-1]} != to_kv in_features {self.context_dim} "
                             "(the reference raises the same shape error, SURVEY note N1)")
        xn = self.norm(x2d)
        ctx2d = self.context_norm(ctx2d)
        q = Fn.LinearBf16Fn.apply(xn, None, self.to_q.weight, self)
        kv = Fn.LinearBf16Fn.apply(ctx2d, None, self.to_kv.weight, self)
        o = Fn.AttentionXFn.apply(q.view(B * n * h, 64), kv, B, 1, n * h, n_ctx, self.scale)
        y = Fn.LinearBf16Fn.apply(o.view(B * n, h * 64), residual, self.to_out.weight, self)
        if self.ff is not None:
            f = Fn.LinearBf16Fn.apply(xn, None, self.ff[0].weight, self)
            y = Fn.LinearBf16Fn.apply(self.ff[1](f), y, self.ff[2].weight, self, (f, 0, f.shape[1] // 2))
        return y


class CoCaForItemAlignment(HipModule):
    """reference multimodal.py:936-1045.  ensemble == "sum": text CLS + image CLS -> two-tower head.

    Note N1: the headline pairing roberta_large (1024-d) + ViT-B/16 (768-d) raises a shape error
    in the reference (multimodal.py:1015 adds a 1024-d and a 768-d vector).  When the two widths differ this
    class inserts one Linear(image_dim -> hidden_size) on the image CLS (`img_proj`, a documented deviation
    needed to run the named benchmark config at all); with equal widths (coca_base + ViT-B, coca_large + ViT-L,
    the reference's working pairings) the module does not exist and the arithmetic is the reference's."""

    def __init__(self, config, image_encoder=None, text_encoder=None):
        super().__init__()
        self.config = config
        self.ensemble = config.ensemble
        self.num_labels = config.num_labels
        self.coca = CoCaModel(config, image_encoder, text_encoder)
        img_dim = getattr(image_encoder, "num_features", config.hidden_size)
        if config.ensemble == "cross_attn":
            # reference multimodal.py:946-961
            self.multimodal_layers = nn.ModuleList([])
            dh = config.hidden_size // config.num_attention_heads_multimodal
            for _ in range(config.num_hidden_layers_multimodal):
                self.multimodal_layers.append(nn.ModuleList([
                    Residual(ParallelTransformerBlock(dim=config.hidden_size, dim_head=dh, heads=config.num_attention_heads_multimodal,
                                                      ff_mult=config.feedforward_multiplication_multimodal, is_decoding=False)),
                    Residual(CrossAttention(dim=config.hidden_size, dim_head=dh, heads=config.num_attention_heads_multimodal,
                                            parallel_ff=True, ff_mult=config.feedforward_multiplication_multimodal))]))
        if img_dim != config.hidden_size and config.ensemble != "cross_attn":
            self.img_proj = nn.Linear(img_dim, config.hidden_size)
            nn.init.normal_(self.img_proj.weight, std=getattr(config, "initializer_range", 0.02))
            nn.init.zeros_(self.img_proj.bias)
        else:
            self.img_proj = None
        if config.classification_method == "vec_sim":
            self.classifier = VecSimClassificationHead(config)
        else:
            self.classifier = TwoTowerClassificationHead(config.hidden_size, dropout=config.hidden_dropout_prob, num_labels=config.num_labels)
            nn.init.normal_(self.classifier.out_proj.weight, std=getattr(config, "initializer_range", 0.02))
            nn.init.zeros_(self.classifier.out_proj.bias)
        self.loss_fct = make_loss(config)
        adopt(self, image_encoder, text_encoder)

    def forward(self, input_ids_1, attention_mask_1, token_type_ids_1, position_ids_1, images_1, input_ids_2, attention_mask_2,
                token_type_ids_2, position_ids_2, images_2, labels=None):
        self.ensure_arena()
        B, L = input_ids_1.shape
        if self.ensemble == "cross_attn":
            return self._forward_cross_attn(input_ids_1, attention_mask_1, token_type_ids_1, position_ids_1, images_1, labels)
        cat = lambda a, b: None if a is None else torch.cat((a, b), dim=0)
        # both items of a pair go through each shared-weight encoder as one 2B batch
        # The two towers are independent until the head.  IA_TOWER_STREAMS=1 runs the image tower on a second HIP stream so
        # that one tower's kernel tails (last partial round of tiles, epilogue drains, HBM-bound LayerNorm tails) fill with
        # the other's work: +3.5 % pairs/s on the bench step (autograd replays each tower's backward on the stream its
        # forward used).  Off by default: concurrent kernels stretch each other's wall time, so per-kernel timings (the
        # bench's roofline leg, rocprofv3 averages) stop describing the kernels themselves.
        two_streams = TOWER_STREAMS and images_1.is_cuda
        images = (images_1, images_2)               # run as one 2B batch; the patch gather reads the two tensors in turn (no fp32 concat)
        cls_only = self.reads_cls_only()

        def image_tower():
            img_tok = self.coca.embed_image(images, cls_only=cls_only)                                                                  # [2B, N, Hi] bf16
            i_cls = self.coca.img_encoder.forward_head(img_tok, pre_logits=True)                                   # [2B, Hi] fp32
            if self.img_proj is not None:
                i_cls = Fn.LinearSmallFn.apply(i_cls, self.img_proj.weight, self.img_proj, ACT_NONE)
            return i_cls
        if two_streams:
            main = torch.cuda.current_stream()
            side = self.__dict__.get("_side_stream")
            if side is None:
                side = self.__dict__["_side_stream"] = torch.cuda.Stream()
                self.param_arena.side_streams.append(side)
            side.wait_stream(main)
            for im in images:
                im.record_stream(side)
            with torch.cuda.stream(side):
                i_cls = image_tower()
        else:
            i_cls = image_tower()
        txt = self.coca.embed_text(cat(input_ids_1, input_ids_2), cat(attention_mask_1, attention_mask_2),
                                   cat(token_type_ids_1, token_type_ids_2), cat(position_ids_1, position_ids_2),
                                   cls_only_read=cls_only)                                                         # [2B, L, H]
        H = txt.shape[-1]
        dev = txt.device
        t_cls = Fn.GatherRowsFn.apply(txt.reshape(2 * B * L, H), self.anchor, cls_rows(2 * B, L, 0, dev), 0.0, 0)   # text_tokens[:, 0]
        if two_streams:
            main.wait_stream(side)
            i_cls.record_stream(main)
        emb = t_cls + i_cls                                                                                          # multimodal.py:1015
        e1, e2 = emb[:B].contiguous(), emb[B:].contiguous()
        return self._finish(e1, e2, labels)

    def reads_cls_only(self):
        """The `sum` head reads text_tokens[:, 0] and the image [CLS] and nothing else of either tower, so the last layer of each may skip
        what follows its attention in every other row (cls_only_read / cls_only: a contract of this caller).  Only for the plain [CLS]
        head on the last layer: every other configuration keeps every row.  A text position 0 that is not attended -- the reference's
        collate never produces one -- is no such row (RobertaEncoder.forward): it stays the row of zeros it is under masked_rows_dead."""
        cfg = self.config
        return (self.ensemble == "sum" and cfg.classification_method == "cls" and str(getattr(cfg, "cls_layers", "1")) == "1"
                and not getattr(cfg, "auxiliary_task", False))

    def _forward_cross_attn(self, input_ids, attention_mask, token_type_ids, position_ids, images, labels):
        """reference multimodal.py:1003-1013.  Quirk A4 (:1013): `embeds_2 = text_tokens_1[:, 0]` — the target embedding is
        the SOURCE item's token, so nothing computed from item 2 reaches the outputs or any gradient; item 2's encoders
        and multimodal layers are therefore not run at all (same outputs, same gradients, half the work)."""
        B, L = input_ids.shape
        img_tok = self.coca.embed_image(images)                                                     # [B, N, Hi] bf16
        txt = self.coca.embed_text(input_ids, attention_mask, token_type_ids, position_ids, padded_rows_matter=True)   # [B, L, H] bf16
        H, N = txt.shape[-1], img_tok.shape[1]
        x = txt.reshape(B * L, H)
        ctx = img_tok.reshape(B * N, img_tok.shape[-1])
        for attn_ff, cross_attn in self.multimodal_layers:
            x = attn_ff(x, B, L)
            x = cross_attn(x, ctx, B, L, N)
        e1 = Fn.GatherRowsFn.apply(x, self.anchor, cls_rows(B, L, 0, x.device), 0.0, 0)            # text_tokens_1[:, 0]
        return self._finish(e1, e1, labels)

    def _finish(self, e1, e2, labels):
        training = self.training and torch.is_grad_enabled()
        if self.config.classification_method == "vec_sim":
            p = self.classifier.drop_p if training else 0.0
            if p > 0:
                e1, e2 = nn.functional.dropout(e1, p, True), nn.functional.dropout(e2, p, True)
            src, tgt, logits, probs2 = self.classifier(e1, e2)
            loss = None
        else:
            p = self.classifier.drop_p if training else 0.0
            if p > 0:
                e1, e2 = nn.functional.dropout(e1, p, True), nn.functional.dropout(e2, p, True)
            ce = self.config.loss_type == "ce"
            src, tgt, logits, probs2, loss = self.classifier(e1, e2, labels if ce else None,
                                                             differentiable_logits=(labels is not None and not ce))
        src, tgt, probs = probs2[:, 0], probs2[:, 1], probs2[:, 1]
        if labels is not None and self.config.loss_type != "ce":
            loss = apply_loss(self.loss_fct, self.config, logits, labels, src, tgt)
        return SequenceClassifierOutput(loss=loss, probs=probs, logits=logits, src_embeds=src, tgt_embeds=tgt)


class _NoLiveCaptionRowFn(torch.autograd.Function):
    """The caption loss of a data-parallel rank none of whose label rows is live while another rank has some: 0, with a zero gradient
    into the hidden states.  It reports the parameters TiedCaptionHeadFn would have touched, at the same place of the backward."""

    @staticmethod
    def forward(ctx, hidden, norm, table):
        ctx.touched, ctx.shape = [p for p in (table, norm.gamma) if p.requires_grad], hidden.shape
        return torch.zeros((), device=hidden.device, dtype=torch.float32)

    @staticmethod
    def backward(ctx, dloss):
        Fn._notify(ctx.touched)
        return torch.zeros(ctx.shape, device=dloss.device, dtype=torch.bfloat16), None, None


class CoCaForPretraining(HipModule):
    """reference multimodal.py:843-933: the text tower and the ViT, `num_hidden_layers_multimodal` pairs of a causal
    ParallelTransformerBlock and a CrossAttention over the image tokens, and `to_logits` = gamma LayerNorm + a Linear tied to the text
    tower's word table.  forward returns caption_loss_weight * CE(logits, labels, ignore_index=pad_id) + contrastive_loss_weight *
    0.5 (CE(sim, arange) + CE(sim^T, arange)), sim = text [CLS] . image [CLS] * exp(temperature).  state_dict keys are the reference's.

    The caption head runs on the rows whose label is not pad (TiedCaptionHeadFn), the contrastive loss in csrc/contrastive.hip.  After a
    forward, `last_losses` holds the two weighted parts (detached) and `caption_live_rows` the number of rows the head ran on.

    Note N2: with labels=None the reference cuts labels = input_ids[:, 2:] against logits of length L - 1 and raises; here
    the labels are input_ids[:, 1:], the next-token shift that makes the shapes agree.  With explicit labels [B, n] the arithmetic is
    the reference's.  `image_tokens` is refused: the reference's embed_image drops it too."""

    def __init__(self, config, image_encoder=None, text_encoder=None, pad_id=0):
        super().__init__()
        if image_encoder is None or text_encoder is None:
            raise ValueError("CoCaForPretraining needs both encoders: the image tower feeds the cross-attention and the contrastive loss")
        if config.vocab_size % 8:
            raise ValueError(f"CoCaForPretraining: vocab_size {config.vocab_size} is not a multiple of 8, which the decoder GEMMs need: resize "
                             f"the word table to {(config.vocab_size + 7) // 8 * 8} rows (pad the vocabulary with unused tokens)")
        img_dim = getattr(image_encoder, "num_features", config.hidden_size)
        if img_dim != config.hidden_size:
            raise ValueError(f"CoCaForPretraining: image width {img_dim} != hidden_size {config.hidden_size}: the contrastive product and "
                             "the cross-attention both need equal widths (the reference's einsum raises there), and no projection is invented")
        self.config = config
        self.pad_id = pad_id
        self.caption_loss_weight = config.caption_loss_weight
        self.contrastive_loss_weight = config.contrastive_loss_weight
        self.coca = CoCaModel(config, image_encoder, text_encoder)
        self.temperature = nn.Parameter(torch.Tensor([1.]))
        self.multimodal_layers = nn.ModuleList([])
        dh = config.hidden_size // config.num_attention_heads_multimodal
        for _ in range(config.num_hidden_layers_multimodal):
            self.multimodal_layers.append(nn.ModuleList([
                Residual(ParallelTransformerBlock(dim=config.hidden_size, dim_head=dh, heads=config.num_attention_heads_multimodal,
                                                  ff_mult=config.feedforward_multiplication_multimodal, is_decoding=True)),
                Residual(CrossAttention(dim=config.hidden_size, dim_head=dh, heads=config.num_attention_heads_multimodal,
                                        parallel_ff=True, ff_mult=config.feedforward_multiplication_multimodal))]))
        # `to_logits.1.weight` is the word table itself, the same Parameter: the arena holds it once
        self.to_logits = nn.Sequential(LayerNorm(config.hidden_size), _TiedDecoder(text_encoder.embeddings.word_embeddings.weight))
        self.last_losses, self.caption_live_rows = None, None
        self._dp = None          # set_data_parallel: (process group,)
        adopt(self, image_encoder, text_encoder)

    def encode(self, input_ids, attention_mask, token_type_ids, position_ids, images):
        """-> (text tokens behind the multimodal layers [B n, H] bf16, text [CLS] embeddings [B, H] fp32, image [CLS] embeddings [B, H]
        fp32): everything in front of the two losses"""
        B, n = input_ids.shape
        img_tok = self.coca.embed_image(images)                                                     # [B, N, H] bf16
        i_cls = self.coca.img_encoder.forward_head(img_tok, pre_logits=True)                        # [B, H] fp32
        # the multimodal layers attend over all n text positions with no padding mask: the padded rows are read
        txt = self.coca.embed_text(input_ids, attention_mask, token_type_ids, position_ids, padded_rows_matter=True)   # [B, n, H] bf16
        H, N = txt.shape[-1], img_tok.shape[1]
        x = txt.reshape(B * n, H)
        t_cls = Fn.GatherRowsFn.apply(x, self.anchor, cls_rows(B, n, 0, x.device), 0.0, 0)          # last_hidden[:, 0]
        ctx = img_tok.reshape(B * N, H)
        for attn_ff, cross_attn in self.multimodal_layers:
            x = attn_ff(x, B, n)
            x = cross_attn(x, ctx, B, n, N)
        return x, t_cls, i_cls

    def forward(self, input_ids, attention_mask, token_type_ids, position_ids, images=None, image_tokens=None, labels=None):
        if image_tokens is not None:
            raise NotImplementedError("CoCaForPretraining: precomputed image_tokens are not supported (the reference's embed_image ignores "
                                      "them and fails on the missing image embeddings)")
        if images is None:
            raise ValueError("CoCaForPretraining: images are required")
        self.ensure_arena()
        if labels is None:
            labels = input_ids[:, 1:]
            input_ids, attention_mask = input_ids[:, :-1].contiguous(), attention_mask[:, :-1].contiguous()
            token_type_ids, position_ids = token_type_ids[:, :-1].contiguous(), position_ids[:, :-1].contiguous()
        B, n = input_ids.shape
        if tuple(labels.shape) != (B, n):
            raise ValueError(f"CoCaForPretraining: labels {tuple(labels.shape)} do not match the {B} x {n} logits")
        x, t_cls, i_cls = self.encode(input_ids, attention_mask, token_type_ids, position_ids, images)
        flat = labels.reshape(-1).to(torch.long)
        rows = (flat != self.pad_id).nonzero(as_tuple=False).squeeze(1)      # the one host sync of the head: M_live sizes its tensors
        self.caption_live_rows = rows.numel()
        if self._dp is not None:
            return self._sharded_losses(x, t_cls, i_cls, flat, rows)
        if rows.numel() == 0:
            caption = torch.full((), float("nan"), device=x.device, dtype=torch.float32)      # torch's mean over no row; no kernel runs with M = 0
        else:
            table = self.to_logits[1].weight
            caption = TiedCaptionHeadFn.apply(x, self, self.to_logits[0], table, rows, flat.index_select(0, rows).contiguous())
        caption = caption * self.caption_loss_weight
        contrastive = Fn.ContrastiveLossFn.apply(t_cls, i_cls, self.temperature) * self.contrastive_loss_weight
        self.last_losses = (caption.detach(), contrastive.detach())
        return caption + contrastive

    def set_data_parallel(self, group=None):
        """From now on a forward is one rank's part of a step that the ranks of `group` (None: the default process group) take on a
        global batch, of which this rank's arguments are a shard: every other item of the global batch is a contrastive negative
        (Fn.ShardedContrastiveLossFn) and the caption loss is the mean over the live label rows of all ranks.  The mean of the ranks'
        losses is the loss of one process on the global batch, and gradients averaged over the ranks are its gradients.
        Every rank must call forward together, each with at least one item; `last_losses` keeps the rank's two parts."""
        if not torch.distributed.is_initialized():
            raise RuntimeError("CoCaForPretraining.set_data_parallel: torch.distributed is not initialised")
        self._dp = (group,)

    def _sharded_losses(self, x, t_cls, i_cls, flat, rows):
        from .. import dist as iadist
        group = self._dp[0]
        world = torch.distributed.get_world_size(group)
        # one small collective: the item counts the contrastive gathers need and the live label rows the caption mean divides by
        counts = iadist.gather_ints([t_cls.shape[0], rows.numel()], group)
        n_live = sum(c[1] for c in counts)
        table = self.to_logits[1].weight
        if n_live == 0:
            caption = torch.full((), float("nan"), device=x.device, dtype=torch.float32)      # as one process: torch's mean over no row
        elif rows.numel() == 0:
            # no live row here, some elsewhere: this rank adds 0 to the caption loss and runs no kernel with M = 0, but its backward still
            # walks the multimodal layers (with a zero gradient), so that every rank starts the gradient buckets in the same order
            caption = _NoLiveCaptionRowFn.apply(x, self.to_logits[0], table)
        else:
            mean = TiedCaptionHeadFn.apply(x, self, self.to_logits[0], table, rows, flat.index_select(0, rows).contiguous())
            # the rank's mean over its n_r live rows -> its share of the global mean, times world (the ranks' losses are averaged)
            caption = mean * (rows.numel() * world / n_live)
        caption = caption * self.caption_loss_weight
        contrastive = Fn.ShardedContrastiveLossFn.apply(t_cls, i_cls, self.temperature, group, [c[0] for c in counts])
        contrastive = contrastive * self.contrastive_loss_weight
        self.last_losses = (caption.detach(), contrastive.detach())
        return caption + contrastive
