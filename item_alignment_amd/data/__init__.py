"""Tensor formats feeding the train step (the reference's collate outputs) and synthetic pair generators."""
from .synthetic import SyntheticCocaPairs, SyntheticItemGraph, one_tower_text, two_tower_text  # noqa: F401
from .datasets import MultimodalDataset, collate_coca  # noqa: F401,E402
from .datasets import RobertaDataset, collate  # noqa: F401,E402
from .graph_files import build_edge_index, read_entity_lines  # noqa: F401,E402
