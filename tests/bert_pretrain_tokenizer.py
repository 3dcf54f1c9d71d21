"""tests/fake_tokenizer.FakeBertTokenizer with `__len__`, which the pre-training example builder draws random token ids from."""
from fake_tokenizer import FakeBertTokenizer


class FakePretrainTokenizer(FakeBertTokenizer):
    def __len__(self):
        return self.vocab_size
