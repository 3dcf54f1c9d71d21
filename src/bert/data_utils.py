"""`from src.bert.data_utils import ...` of the reference: the data layer of item_alignment_amd.data.bert_align."""
from item_alignment_amd.data.bert_align import (read_data, shuffle_pvs_pairs, join_data, get_examples, encode, get_dataloader, show,  # noqa: F401
                                                show_pairs)
