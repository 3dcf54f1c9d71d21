"""`from src.bert.model import BertAlignModel` of the reference: the HIP-engine model of item_alignment_amd.models.bert_align."""
from item_alignment_amd.models.bert_align import BertAlignModel, BertOnlyNSPHead  # noqa: F401
