"""numpy window partition of the SWIN tests, apart from them so that a test without a device can use it too."""
import numpy as np


def windows(x, ws, shift):
    """numpy pad + roll(-shift) + window_partition of [B, H, W, C] -> ([B*nwy*nwx*N, C], validity of each row)."""
    B, H, W, Cc = x.shape
    hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
    p = np.zeros((B, hp, wp, Cc), x.dtype)
    p[:, :H, :W] = x
    valid = np.zeros((B, hp, wp), bool)
    valid[:, :H, :W] = True
    p, valid = np.roll(p, (-shift, -shift), (1, 2)), np.roll(valid, (-shift, -shift), (1, 2))
    part = lambda a: a.reshape(B, hp // ws, ws, wp // ws, ws, -1).transpose(0, 1, 3, 2, 4, 5).reshape(-1, a.shape[-1] if a.ndim == 4 else 1)  # noqa: E731
    return part(p), part(valid[..., None])[:, 0]
