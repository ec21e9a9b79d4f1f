"""What every evaluation pass over a model shares: where the model lives, how a batch of images is looked up, the eval-mode
bracket and the rule that draws which images a score sees.  The scores (``aggregate``, ``quality``, ``density``,
``likelihood``, ``disentangle``) and the solver's writer take these from here; none keeps a copy."""
import contextlib

import numpy as np
import torch


def device_of(model):
    return next(model.parameters()).device


def images(source, idx, device):
    """fp32 ``[len(idx), C, H, W]`` on ``device``: the images of ``source`` at ``idx``.  ``source``: a ``DeviceImageTable``
    (one ``gather`` launch) or a dataset (``__getitem__``; an item is an image or a tuple that starts with one)."""
    if hasattr(source, "gather"):                      # a DeviceImageTable: one launch per batch
        return source.gather(idx)
    items = [source[int(i)] for i in idx]
    return torch.stack([it[0] if isinstance(it, (tuple, list)) else it for it in items], 0).to(device)


@contextlib.contextmanager
def eval_mode(model):
    """``model`` in eval mode and under ``no_grad`` inside the block; its training flag is put back on the way out, on an
    exception too.  The BatchNorm running buffers are not written in eval mode."""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield model
    finally:
        model.train(was_training)


def draw_indices(n, num, seed):
    """int64, ascending: which of ``n`` images a score sees.  All of them when ``num >= n``, otherwise
    ``np.sort(np.random.RandomState(seed).choice(n, num, replace=False))``: a private generator, so equal seeds give
    every score the same images."""
    if int(num) >= n:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.RandomState(seed).choice(n, int(num), replace=False)).astype(np.int64)
