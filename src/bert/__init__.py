"""Drop-in import path of the reference's src/bert package (finetune_bert.py / pred_bert.py: `from src.bert.model import
BertAlignModel`, `from src.bert.data_utils import ...`, `from src.bert.log import LOGGER`): re-exports the MI355X-native
implementations."""
