"""SAM's mask-input prompt (PromptEncoder._embed_masks: Conv2d(1, 4, 2, 2) LayerNorm2d GELU Conv2d(4, 16, 2, 2) LayerNorm2d GELU Conv2d(16, dim, 1)) added to an
image embedding, in plain numpy: the reference of vx_sam_dense_prompt_f16 (csrc/kernels_samdense.hip) and of the mask-input cases of tests/test_gpu_sam_predict.py.
Convolutions as einsum, LayerNorm2d over the channels (biased variance, eps 1e-6), erf GELU. Evaluated in `dtype`: float64 is the reference, float32 numpy's own
evaluation whose distance from it sizes the kernel's allowance. Both apply the kernel's two declared roundings: the 16 stage-2 activations to f16 before the last
product, and the result to f16 (`K`; `raw` is the result before that rounding)."""
import numpy as np
from scipy.special import erf

EPS = 1e-6
MD = "prompt_encoder.mask_downscaling."


def weights(tensors):
    """the ten mask_downscaling tensors of a state dict or of a file's tensors, at the f16 values a file holds, as float64"""
    return {k[len(MD):]: np.asarray(v).astype(np.float16).astype(np.float64) for k, v in tensors.items() if k.startswith(MD)}


def _norm_gelu(x, w, b, dtype):
    mean = x.mean(axis=-1, keepdims=True, dtype=dtype)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True, dtype=dtype)
    y = ((x - mean) / np.sqrt(var + dtype(EPS))) * w.astype(dtype) + b.astype(dtype)
    return (dtype(0.5) * y * (dtype(1) + erf(y / np.sqrt(dtype(2))).astype(dtype))).astype(dtype)


def dense(mask, W, dtype=np.float64):
    """mask [n, 4 res, 4 res] -> (stage-2 activations rounded to f16 [n, res, res, 16], the 1x1 conv of them + bias [n, res, res, dim]), in dtype"""
    x = np.asarray(mask).astype(dtype)
    n, S = x.shape[0], x.shape[1]
    w = {k: v.astype(dtype) for k, v in W.items()}
    a1 = np.einsum("nyaxb,cab->nyxc", x.reshape(n, S // 2, 2, S // 2, 2), w["0.weight"][:, 0]) + w["0.bias"]
    s1 = _norm_gelu(a1.astype(dtype), w["1.weight"], w["1.bias"], dtype)
    a2 = np.einsum("nyaxbi,oiab->nyxo", s1.reshape(n, S // 4, 2, S // 4, 2, 4), w["3.weight"]) + w["3.bias"]
    act = _norm_gelu(a2.astype(dtype), w["4.weight"], w["4.bias"], dtype).astype(np.float16).astype(dtype)
    return act, (np.einsum("nyxk,ok->nyxo", act, w["6.weight"][:, :, 0, 0]) + w["6.bias"]).astype(dtype)


def dense_prompt(mask, W, embed, dtype=np.float64):
    """-> (raw [n, res^2, dim] in dtype = embed [res^2, dim] + the dense prompt, K = raw rounded to f16)"""
    _, d = dense(mask, W, dtype)
    raw = d.reshape(d.shape[0], -1, d.shape[-1]) + np.asarray(embed).astype(dtype)[None]
    return raw, raw.astype(np.float16)


def k1_of(K, pe):
    """what the kernel declares for its second output: f16(K as stored + pe), one float32 add of two f16 values"""
    return (np.asarray(K, np.float16).astype(np.float32) + np.asarray(pe, np.float16).astype(np.float32)[None]).astype(np.float16)
