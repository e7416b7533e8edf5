"""Host arrays and tensors alike as tensors: what the learners do to every leaf of a batch they are handed."""
from __future__ import annotations

import numpy as np
import torch


def to_tensor(x, device=None, dtype=None) -> torch.Tensor:
    """`x` (tensor, array, list) as a tensor; with `device`: moved there as a contiguous `dtype` tensor."""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t if device is None else t.to(device, dtype).contiguous()
