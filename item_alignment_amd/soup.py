"""Uniform model soup, the host-side pass the two model_soup_*.py scripts share (reference model_soup_multimodal.py:223-239,
model_soup_text.py:225-240): the parameters of a model averaged over the checkpoints of several epochs."""
from collections import OrderedDict

import torch


def uniform_soup(model, pattern, epochs):
    """state_dict of the soup: every entry that is a parameter of `model` is the mean over pattern.format(epoch) for the listed epochs,
    every other entry (buffers) comes from the last listed checkpoint, as in the reference.  The sum runs in the checkpoints' own
    dtype, in the order listed."""
    names = set(dict(model.named_parameters()))
    st = OrderedDict()
    for epoch in epochs:
        sd = torch.load(pattern.format(epoch), map_location="cpu")
        for key, val in sd.items():
            if key not in names:
                st[key] = val                      # buffers: the last listed epoch wins
            elif key not in st:
                st[key] = val.clone()
            else:
                st[key] += val
    for key, val in st.items():
        if key in names:
            val /= len(epochs)
    return st


def load_soup(model, st, epochs, logger):
    """the soup into the model; a key the model does not know is an error"""
    missing, unexpected = model.load_state_dict(st, strict=False)
    if unexpected:
        raise RuntimeError(f"unexpected keys in the checkpoints: {unexpected[:5]}")
    logger.info(f"Finished uniform soup on epochs: {epochs}")
