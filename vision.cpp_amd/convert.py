"""Checkpoint -> GGUF conversion for Depth-Anything-V2 (the `transformers` / .safetensors layout), following
the reference's scripts/convert.py:428-475 (convert_depth_anything) and :46-98 (Writer) rule by rule, so that a
file written here is interchangeable with one written by the reference's converter:

  * KV: general.architecture = "depthanything", depthanything.tensor_data_layout = "whcn" (default layout),
    dino.patch_size / dino.embed_dim from the patch-embedding kernel shape, depthanything.image_size = 518,
    dino.n_heads / dino.n_layers / depthanything.feature_layers from the embed dim (384 S, 768 B, 1024 L),
    general.file_type (1 = f16), depthanything.conv2d_weights (indices of OIHW kernels);
  * tensors in state-dict order, names unchanged (< 64 chars); patch-embed and reassemble `projection` kernels
    permuted to NHWC, ConvTranspose (`0.resize`, `1.resize`) untouched, other 2-D conv kernels left OIHW and
    listed in conv2d_weights; cls_token / position_embeddings kept f32, everything else cast to f16.
The third-party `gguf` package the reference uses is not required (own writer, vision.cpp_amd/gguf.py)."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from .gguf import GGUFWriter
from .synth import gguf_tensors

_VARIANTS = {384: (6, 12, [2, 5, 8, 11]), 768: (12, 12, [2, 5, 8, 11]), 1024: (16, 24, [4, 11, 17, 23])}


def convert_depth_anything(state_dict: dict[str, np.ndarray], out_path: str | Path, image_size: int = 518) -> Path:
    if "pretrained.cls_token" in state_dict:
        raise ValueError("The converter is written for the transformers (.safetensors) version of the model; "
                         "the original weights (.pth) are not supported")  # convert.py:437-440
    key = "backbone.embeddings.patch_embeddings.projection.weight"
    if key not in state_dict:
        raise ValueError(f"not a Depth-Anything checkpoint: {key} missing")
    shape = state_dict[key].shape
    embed_dim, patch = int(shape[0]), int(shape[2])
    w = GGUFWriter(out_path, "depthanything")
    w.add_string("depthanything.tensor_data_layout", "whcn")
    w.add_int32("dino.patch_size", patch)
    w.add_int32("dino.embed_dim", embed_dim)
    w.add_int32("depthanything.image_size", image_size)
    if embed_dim in _VARIANTS:
        heads, layers, feats = _VARIANTS[embed_dim]
    else:  # non-standard (test-size) models: head_dim 64, taps at the four quarter points
        layers = 1 + max(int(k.split(".")[3]) for k in state_dict if k.startswith("backbone.encoder.layer."))
        heads, feats = max(1, embed_dim // 64), [layers * (i + 1) // 4 - 1 for i in range(4)]
    w.add_int32("dino.n_heads", heads)
    w.add_int32("dino.n_layers", layers)
    w.add_array_i32("depthanything.feature_layers", feats)
    tensors, conv2d = gguf_tensors({k: np.asarray(v, dtype=np.float32) for k, v in state_dict.items()})
    w.add_uint32("general.quantization_version", 2)
    w.add_uint32("general.file_type", 1)
    w.add_array_i32("depthanything.conv2d_weights", conv2d)
    for name, t in tensors.items():
        w.add_tensor(name, t)
    w.write()
    return Path(out_path)


def load_safetensors(path: str | Path) -> dict[str, np.ndarray]:
    from safetensors.numpy import load_file  # plain tensor container, nothing is executed from the file

    return load_file(str(path))


# ---- ESRGAN / Real-ESRGAN (reference scripts/convert.py:504-527, convert_esrgan) ---------------------------------
#
# The reference loads any ESRGAN checkpoint through `spandrel`, which normalises the zoo's key layouts to the original
# ESRGAN ("old arch") names `model.<i>...`, then writes: esrgan.scale, esrgan.block_count, esrgan.filter_count,
# esrgan.tensor_data_layout = "whcn", every 4-D kernel left OIHW and listed in esrgan.conv2d_weights, floats -> f16.
# spandrel is not available here; the one renaming it performs for RRDBNet files (the BasicSR / Real-ESRGAN "new arch"
# names) is restated below, so `RealESRGAN_x4plus`-style state dicts and old-arch ones both convert.

_NEW_ARCH_FIXED = {"conv_first": "model.0", "conv_body": None, "trunk_conv": None, "conv_hr": None, "HRconv": None, "conv_last": None}


def esrgan_to_old_arch(sd: dict[str, np.ndarray]) -> dict[str, np.ndarray]:
    """BasicSR RRDBNet names (conv_first, body.N.rdbK.convJ, conv_body, conv_up1/2, conv_hr, conv_last) or the early
    'RRDB_trunk' names -> `model.0`, `model.1.sub.N.RDBK.convJ.0`, `model.1.sub.<nb>`, `model.3/6`, `model.8`, `model.10`."""
    if any(k.startswith("model.0.") for k in sd):
        return dict(sd)
    import re

    blocks = set()
    for k in sd:
        m = re.match(r"(?:body|RRDB_trunk)\.(\d+)\.", k)
        if m:
            blocks.add(int(m.group(1)))
    if not blocks or not any(k.startswith("conv_first.") for k in sd):
        raise ValueError("not an RRDBNet (ESRGAN) state dict: neither model.0.* nor conv_first.* / body.* keys")
    nb = max(blocks) + 1
    ups = sorted({k.split(".")[0] for k in sd if re.match(r"(conv_up|upconv)\d+\.", k)}, key=lambda s: int(re.sub(r"\D", "", s)))
    seq = 2 + 3 * len(ups)
    top = {"conv_first": "model.0", "conv_body": f"model.1.sub.{nb}", "trunk_conv": f"model.1.sub.{nb}",
           "conv_hr": f"model.{seq}", "HRconv": f"model.{seq}", "conv_last": f"model.{seq + 2}"}
    for i, u in enumerate(ups):
        top[u] = f"model.{3 + 3 * i}"
    out: dict[str, np.ndarray] = {}
    for k, v in sd.items():
        head, _, rest = k.partition(".")
        if head in top:
            out[f"{top[head]}.{rest}"] = v
            continue
        m = re.match(r"(?:body|RRDB_trunk)\.(\d+)\.(?:rdb|RDB)(\d)\.conv(\d)\.(weight|bias)$", k)
        if not m:
            raise ValueError(f"unexpected key in RRDBNet state dict: {k}")
        out[f"model.1.sub.{m.group(1)}.RDB{m.group(2)}.conv{m.group(3)}.0.{m.group(4)}"] = v
    return out


def convert_esrgan(state_dict: dict[str, np.ndarray], out_path: str | Path) -> Path:
    sd = {k: np.asarray(v) for k, v in esrgan_to_old_arch(state_dict).items()}
    nb = 1 + max(int(k.split(".")[3]) for k in sd if k.startswith("model.1.sub.") and ".RDB" in k)
    nf = int(sd["model.0.weight"].shape[0])
    if sd["model.0.weight"].shape[1] != 3:
        raise ValueError("RealESRGAN models with pixel shuffle are not supported yet.")  # convert.py:513-514
    tops = sorted({int(k.split(".")[1]) for k in sd if k.count(".") == 2 and k.startswith("model.")})  # 0, 3, 6, 8, 10 for x4
    n_up = len(tops) - 3  # first, HR and last convs are always there
    if n_up < 0 or tops[-1] != 2 + 3 * n_up + 2:
        raise ValueError(f"unexpected top-level layout of the RRDBNet sequence: {tops}")
    # order tensors as torch's state_dict of the old-arch module does (the conv2d index list depends on it)
    def order(k):
        p = k.split(".")
        return (int(p[1]), int(p[3]) if p[1] == "1" else 0, p[4] if p[1] == "1" and len(p) > 5 else "", k.replace("weight", "0"))
    from .synth import esrgan_gguf_tensors

    tensors, conv2d = esrgan_gguf_tensors({k: sd[k].astype(np.float32) for k in sorted(sd, key=order)})
    w = GGUFWriter(out_path, "esrgan")
    w.add_string("esrgan.tensor_data_layout", "whcn")
    w.add_int32("esrgan.scale", 1 << n_up)
    w.add_int32("esrgan.block_count", nb)
    w.add_int32("esrgan.filter_count", nf)
    w.add_uint32("general.quantization_version", 2)
    w.add_uint32("general.file_type", 1)
    w.add_array_i32("esrgan.conv2d_weights", conv2d)
    for name, t in tensors.items():
        w.add_tensor(name, t)
    w.write()
    return Path(out_path)


def convert_sam(state_dict: dict[str, np.ndarray], out_path: str | Path) -> Path:
    """MobileSAM checkpoint (image_encoder.* = TinyViT-5M, prompt_encoder.*, mask_decoder.*) -> GGUF with the on-disk contract
    of the reference's convert_sam (scripts/convert.py:204-262): BatchNorm fused into `<conv>.c.weight/.c.bias`, `local_conv`
    always NHWC and unlisted, `attention_biases_indexed`, neck convs listed, mask_decoder. -> dec., _token_to_image /
    _image_to_token -> _t2i / _i2t, iou / mask tokens f32, dense positional embedding precomputed."""
    from .synth import mobile_sam_gguf_tensors

    enc = {k[len("image_encoder."):]: np.asarray(v, np.float32) for k, v in state_dict.items()
           if k.startswith("image_encoder.") and not k.endswith("num_batches_tracked") and "attention_bias_idxs" not in k}
    dec = {k: np.asarray(v, np.float32) for k, v in state_dict.items() if not k.startswith("image_encoder.")}
    if "patch_embed.seq.0.c.weight" not in enc or "mask_decoder.iou_token.weight" not in dec:
        raise ValueError("not a MobileSAM state dict (image_encoder.patch_embed / mask_decoder.iou_token missing)")
    tensors, conv2d = mobile_sam_gguf_tensors(enc, dec)
    too_long = [n for n in tensors if len(n) >= 64]  # GGML_MAX_NAME (convert.py:58-59)
    if too_long:
        raise ValueError(f"tensor name too long for GGUF: {too_long[0]}")
    w = GGUFWriter(out_path, "mobile-sam")
    w.add_string("mobile-sam.tensor_data_layout", "whcn")
    w.add_uint32("general.quantization_version", 2)
    w.add_uint32("general.file_type", 1)
    w.add_array_i32("mobile-sam.conv2d_weights", conv2d)
    for name, t in tensors.items():
        w.add_tensor(name, t)
    w.write()
    return Path(out_path)


# ---- YOLOv9t (reference src/visp/arch/yolov9t.cpp; the reference ships no converter for this family) ------------------------

def fold_yolov9t(state_dict: dict[str, np.ndarray], bn_eps: float = 1e-3) -> dict[str, np.ndarray]:
    """A torch state dict of the tiny model (e.g. the yolov9t_converted.pth the reference's scripts/yolov9t.py saves) -> the tensor
    set the graph reads: every `<p>.bn.*` folded into `<p>.conv.weight` / `<p>.conv.bias` (Conv is always called with bn=false,
    yolov9t.cpp:78-120), the head renamed from `model.22.` to `detect.`, the fixed DFL projection (dfl.conv.weight = arange(16)) and
    num_batches_tracked dropped. bn_eps: the checkpoint's BatchNorm eps (1e-3 for ultralytics). A dict that is already folded passes."""
    sd = {k: np.asarray(v) for k, v in state_dict.items()}
    out: dict[str, np.ndarray] = {}
    for k, v in sd.items():
        if k.startswith("model.22."):
            k = "detect." + k[len("model.22."):]
        if ".dfl." in k or k.endswith("num_batches_tracked") or ".bn." in k:
            continue
        out[k] = v.astype(np.float32)
    for k, v in sd.items():
        if not k.endswith(".bn.weight"):
            continue
        p = k[: -len(".bn.weight")]
        gamma, beta = v.astype(np.float64), sd[p + ".bn.bias"].astype(np.float64)
        mean, var = sd[p + ".bn.running_mean"].astype(np.float64), sd[p + ".bn.running_var"].astype(np.float64)
        q = "detect." + p[len("model.22."):] if p.startswith("model.22.") else p
        w = sd[p + ".conv.weight"].astype(np.float64)
        b = sd[p + ".conv.bias"].astype(np.float64) if p + ".conv.bias" in sd else np.zeros(w.shape[0])
        s = gamma / np.sqrt(var + bn_eps)
        out[q + ".conv.weight"] = (w * s[:, None, None, None]).astype(np.float32)
        out[q + ".conv.bias"] = ((b - mean) * s + beta).astype(np.float32)
    return out


def convert_yolov9t(state_dict: dict[str, np.ndarray], out_path: str | Path, bn_eps: float = 1e-3) -> Path:
    """fold_yolov9t, then GGUF: general.architecture = "yolov9t", yolov9t.tensor_data_layout = "whcn", conv kernels f16 OIHW listed
    in yolov9t.conv2d_weights, biases f32, general.file_type 1 (f16), tensors in state-dict order."""
    sd = fold_yolov9t(state_dict, bn_eps)
    if "detect.cv3.0.2.weight" not in sd:
        raise ValueError("not a YOLOv9t state dict: no detect.cv3.0.2.weight (or model.22.cv3.0.2.weight)")
    w = GGUFWriter(out_path, "yolov9t")
    w.add_string("yolov9t.tensor_data_layout", "whcn")
    w.add_uint32("general.quantization_version", 2)
    w.add_uint32("general.file_type", 1)
    conv2d: list[int] = []
    tensors: dict[str, np.ndarray] = {}
    for name, t in sd.items():
        if name.endswith(".weight") and t.ndim == 4:
            conv2d.append(len(tensors))
            tensors[name] = t.astype(np.float16)
        else:
            tensors[name] = t.astype(np.float32)
    w.add_array_i32("yolov9t.conv2d_weights", conv2d)
    for name, t in tensors.items():
        w.add_tensor(name, t)
    w.write()
    return Path(out_path)
