"""`from src.bert.log import LOGGER` of the reference: the logger the BERT pair classifier's data layer and scripts write to."""
from item_alignment_amd.data.bert_align import LOGGER  # noqa: F401
