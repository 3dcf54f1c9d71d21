"""BertAlignModel on the HIP engine: the "BERT-NSP" pair classifier the reference's finetune_bert.py trains and pred_bert.py applies
(reference src/bert/model.py:160-218).  Five fields of a product pair -- pvs, title, cate, cate_path, industry_name, each tokenised as
a sentence pair -- go through the SAME BERT encoder; the five pooled outputs are summed and a Linear(H, 2) next-sentence head
classifies the sum.  The state_dict keys are those of transformers.BertForNextSentencePrediction (`bert.*`, `cls.seq_relationship.*`),
so the model starts from a plain BERT directory or from what bert_pretrain.py writes.

The reference runs five padded forward passes (512, 150, 20, 50 and 20 positions at its own settings).  Here the valid tokens of all
5 B sequences run as ONE ragged batch (RobertaModel._forward_packed): no row of padding is embedded, projected or attended to.
That is sound for this model because its inputs come from the tokenizer, whose attention mask marks every real token, [CLS] and [SEP]
included -- the pooler reads the first valid token of each sequence, and that is its [CLS].  (bert_pretrain.py's features give [CLS]
and [SEP] mask 0 and that model has to run dense: models/bert_pretrain.py.)

Not built: the adversarial modes (FREE / PGD / MIX noise added to the pvs and title embeddings).  The reference switches them off by a
constant in its main(); a noise argument raises NotImplementedError here.
"""
import os

import torch
from torch import nn

from . import functional as Fn
from .base import ACT_TANH, HipModule
from .bert_pretrain import init_the_bert_way, save_bert_pretrained
from .text import PretrainedMixin, RobertaModel

FIELDS = ("pvs", "title", "cate", "cate_path", "industry_name")      # the order of the packed batch (and of the data layer's tensors)


class BertOnlyNSPHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.seq_relationship = nn.Linear(config.hidden_size, 2)


class BertAlignModel(HipModule, PretrainedMixin):
    """model(pvs_input_ids=..., pvs_token_type_ids=..., pvs_attention_mask=..., title_..., cate_..., cate_path_..., industry_name_...,
    next_sentence_label=None) -> [pool_out, seq_relationship_score] and, with labels, the mean cross-entropy as a third element.
    pool_out: fp32 [B, H], the sum over the five fields of tanh(W_p h_CLS + b_p)."""

    def __init__(self, config=None):
        super().__init__()
        if getattr(config, "pad_token_id", 0) is None:
            config.pad_token_id = 0
        self.config = config
        self.num_labels = 2
        self.bert = RobertaModel(config)
        self.cls = BertOnlyNSPHead(config)
        init_the_bert_way(self)

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, config=None, **kwargs):
        """from_pretrained(dir), as the reference calls it: the configuration is the directory's config.json unless one is passed"""
        if config is None:
            from ..cli_common import load_config
            config = load_config(os.path.join(str(pretrained_model_name_or_path), "config.json"))
        return super().from_pretrained(pretrained_model_name_or_path, *model_args, config=config, **kwargs)

    def save_pretrained(self, save_directory):
        save_bert_pretrained(self, save_directory)

    def get_sim_eval_weight(self):
        """score = weight . pool_out + bias is logit[1] - logit[0] (reference model.py:170-174)"""
        w = self.cls.seq_relationship.weight.detach().cpu()
        b = self.cls.seq_relationship.bias.detach().cpu()
        return w[1] - w[0], b[1] - b[0]

    def forward(self,
                pvs_input_ids=None, pvs_token_type_ids=None, pvs_attention_mask=None,
                title_input_ids=None, title_token_type_ids=None, title_attention_mask=None,
                cate_input_ids=None, cate_token_type_ids=None, cate_attention_mask=None,
                cate_path_input_ids=None, cate_path_token_type_ids=None, cate_path_attention_mask=None,
                industry_name_input_ids=None, industry_name_token_type_ids=None, industry_name_attention_mask=None,
                next_sentence_label=None, pvs_noise=None, title_noise=None):
        if pvs_noise is not None or title_noise is not None:
            raise NotImplementedError("BertAlignModel: the adversarial modes (pvs_noise / title_noise) are not built; the reference's "
                                      "main() switches them off (adversarial_train = False)")
        self.ensure_arena()
        given = locals()
        fields = []
        for name in FIELDS:
            ids, tts, mask = (given[f"{name}_{k}"] for k in ("input_ids", "token_type_ids", "attention_mask"))
            if ids is None:
                raise ValueError(f"BertAlignModel: {name}_input_ids is missing (all five fields are summed)")
            B, L = ids.shape
            if fields and B != fields[0][0].shape[0]:
                raise ValueError(f"BertAlignModel: {name}_input_ids has {B} rows, pvs_input_ids {fields[0][0].shape[0]}")
            ids = ids.to(torch.long)
            tts = torch.zeros_like(ids) if tts is None else tts.to(torch.long)
            mask = torch.ones_like(ids) if mask is None else mask
            # BERT's absolute positions: every token's own place in its padded sequence
            pos = torch.arange(L, device=ids.device, dtype=torch.long).unsqueeze(0).expand(B, L)
            fields.append((ids, tts, pos, mask))
        B = fields[0][0].shape[0]
        hidden, _idx, cu = self.bert._forward_packed(fields, strict=True)
        # the first valid token of every sequence: its [CLS] (strict=True has checked that position 0 is valid)
        cls_h = Fn.GatherRowsFn.apply(hidden[-1], self.anchor, cu[:-1].contiguous(), 0.0, 0)
        pooled = Fn.LinearSmallFn.apply(cls_h, self.bert.pooler.dense.weight, self.bert.pooler.dense, ACT_TANH)       # [5 B, H]
        pool_out = pooled.view(len(FIELDS), B, -1).sum(dim=0)
        labels = None if next_sentence_label is None else next_sentence_label.reshape(-1).to(torch.long).contiguous()
        score, _probs, loss = Fn.PairHeadCEFn.apply(pool_out, None, self.cls.seq_relationship, labels)
        output = [pool_out, score]
        if labels is not None:
            output.append(loss)
        return output
