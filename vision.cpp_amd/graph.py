"""Graph layer: Python face of the `visp_graph_*` C entries (include/visp_c_api.h), with the reference's builder vocabulary --
`ModelRef` = `model_ref` (include/visp/ml.h:199-245: weights by name under a prefix, `m["sub"]`, `m[i]`), the `nn.h` functions
(`linear`, `layer_norm`, `conv_2d`, `conv_transpose_2d`, `patch_embed`, `attention`), `slice_` / `concat` / `interpolate`
(ml.cpp:746-788) and the raw element-wise / shape ops the reference's arch code calls on ggml directly. Shapes are ggml's ne
order (ne[0] contiguous); 2D maps are CWHN (`model_build_flag::cwhn`), so the layout helpers of nn.h are identities here.

`depthany_predict` below is Depth-Anything-V2 written against this layer the way the reference's arch code is
(src/visp/arch/dino.cpp, src/visp/arch/depth-anything.cpp): the generic path through the executor, next to the hand-scheduled
step of csrc/depthany.cpp that the benchmark measures."""
from __future__ import annotations

import ctypes
import math
from ctypes import byref, c_float, c_int32, c_int64, c_void_p

import numpy as np

from . import _lib as lib
from ._lib import check, get_lib

F32, F16, U8, I32 = 0, 1, 24, 26
# OP_LINEAR ... OP_ROPE: enum visp_graph_op of include/visp_c_api.h, its names without the VISP_ prefix
globals().update({k.removeprefix("VISP_"): v for k, v in lib.C_API_DECLS.enums["visp_graph_op"].items()})
SCALE_MODE_NEAREST, SCALE_MODE_BILINEAR, SCALE_MODE_BICUBIC, SCALE_FLAG_ALIGN_CORNERS = 0, 1, 2, 256  # ggml's values (ml.cpp:782-788)
SLICE_ALL = (0, 2**62, 1)


def _ne(shape) -> tuple[int, int, int, int]:
    shape = tuple(int(v) for v in shape)
    return shape + (1,) * (4 - len(shape))


class Tensor:
    """A handle into its graph (`visp::tensor`)."""

    def __init__(self, graph: "Graph", index: int):
        self.graph, self.index = graph, index

    @property
    def ne(self) -> tuple[int, int, int, int]:
        return self.graph.info(self)[1]

    @property
    def dtype(self) -> int:
        return self.graph.info(self)[0]

    @property
    def is_constant(self) -> bool:
        return self.graph.info(self)[2]

    def __repr__(self):
        return f"Tensor({self.index}, ne={self.ne})"


class Weights:
    """`model_weights` (ml.h:126-149): a model's tensors by name. Device images are made by the first graph that uses a tensor and shared
    by every later graph over the same weights."""

    def __init__(self, path=None):
        self._api = get_lib()
        h = c_void_p()
        if path is None:
            check(self._api.visp_weights_create(byref(h)))
        else:
            check(self._api.visp_weights_load(lib.path_to_char_p(path), byref(h)))
        self._handle = h

    def add(self, name: str, array: np.ndarray, dtype: int = F16):
        a = np.ascontiguousarray(array, dtype=np.float32)
        check(self._api.visp_weights_add(self._handle, name.encode(), dtype, (c_int64 * 4)(*_ne(a.shape[::-1])), a.ctypes.data_as(c_void_p)))

    def __del__(self):
        if getattr(self, "_handle", None):
            self._api.visp_weights_destroy(self._handle)
            self._handle = None


class Graph:
    """`compute_graph` over a model's weights. `device=None`: lower and plan only (no GPU needed)."""

    def __init__(self, device=None, weights: Weights | None = None):
        self._api = get_lib()
        self._device = device  # kept alive; bound when the graph is allocated (compute_graph_allocate(graph, backend))
        self._weights = weights
        if weights is not None and device is not None:
            weights._device = device  # the weights' device images are freed on the device they were made on: it outlives a Weights that outlives its graphs
        h = c_void_p()
        check(self._api.visp_graph_create(weights._handle if weights is not None else None, byref(h)))
        self._handle = h

    def __del__(self):
        if getattr(self, "_handle", None):
            self._api.visp_graph_destroy(self._handle)
            self._handle = None

    # ---- weights
    def add_weight(self, name: str, array: np.ndarray, dtype: int = F16) -> Tensor:
        """`array` in torch / numpy index order (slowest first): its reversed shape is the ggml ne. Also how a constant that is not a file
        weight enters the graph (a precomputed mask or index); `get_tensor(name)` finds it again."""
        a = np.ascontiguousarray(array, dtype=np.int32 if dtype == I32 else np.float32)  # I32: an index constant (get_rows)
        ne = (c_int64 * 4)(*_ne(a.shape[::-1]))
        out = c_int32()
        check(self._api.visp_graph_add_weight(self._handle, name.encode(), dtype, ne, a.ctypes.data_as(c_void_p), byref(out)))
        return Tensor(self, out.value)

    def find(self, name: str) -> Tensor | None:
        out = c_int32()
        check(self._api.visp_graph_find_weight(self._handle, name.encode(), byref(out)))
        return Tensor(self, out.value) if out.value >= 0 else None

    # ---- nodes
    def input(self, ne, dtype: int = F32, name: str = "input") -> Tensor:
        out = c_int32()
        check(self._api.visp_graph_input(self._handle, dtype, (c_int64 * 4)(*_ne(ne)), name.encode(), byref(out)))
        return Tensor(self, out.value)

    def op(self, op: int, src, iparams=(), fparams=()) -> Tensor:
        srcs = (c_int32 * len(src))(*[t.index for t in src])
        ip = (c_int64 * max(1, len(iparams)))(*[int(v) for v in iparams])
        fp = (c_float * max(1, len(fparams)))(*[float(v) for v in fparams])
        out = c_int32()
        check(self._api.visp_graph_op(self._handle, op, srcs, len(src), ip, len(iparams), fp, len(fparams), byref(out)))
        return Tensor(self, out.value)

    def set_name(self, t: Tensor, name: str) -> Tensor:
        check(self._api.visp_graph_set_name(self._handle, t.index, name.encode()))
        return t

    def get_tensor(self, name: str) -> Tensor | None:
        out = c_int32()
        check(self._api.visp_graph_get_tensor(self._handle, name.encode(), byref(out)))
        return Tensor(self, out.value) if out.value >= 0 else None

    def output(self, t: Tensor, name: str = "output") -> Tensor:
        check(self._api.visp_graph_output(self._handle, t.index, name.encode()))
        return t

    def info(self, t: Tensor):
        dtype, const = c_int32(), c_int32()
        ne = (c_int64 * 4)()
        check(self._api.visp_graph_tensor_info(self._handle, t.index, byref(dtype), ne, byref(const)))
        return dtype.value, tuple(ne), bool(const.value)

    def read_constant(self, t: Tensor) -> np.ndarray:
        ne = self.info(t)[1]
        out = np.empty(ne[::-1], np.float32)
        check(self._api.visp_graph_read_constant(self._handle, t.index, out.ctypes.data_as(c_void_p), out.size))
        return out

    # ---- execution
    def set_fused_models(self, enable: bool):
        """Before allocate(). True (default): the lowering may map whole node groups onto the kernels written for them; False: one launch per
        epilogue-fused node on f16 activations."""
        check(self._api.visp_graph_set_fused_models(self._handle, int(enable)))

    def allocate(self):
        check(self._api.visp_graph_allocate(self._handle, self._device._handle if self._device is not None else None))

    def use_hip_graph(self, enable: bool = True):
        check(self._api.visp_graph_use_hip_graph(self._handle, 1 if enable else 0))

    def compute(self):
        check(self._api.visp_graph_compute(self._handle))

    def set(self, t: Tensor, array: np.ndarray):
        dtype, ne, _ = self.info(t)
        a = np.ascontiguousarray(array, dtype={F32: np.float32, U8: np.uint8, I32: np.int32}.get(dtype, np.float16))
        if a.size != int(np.prod(ne)):
            raise ValueError(f"tensor {t} takes {int(np.prod(ne))} elements, got {a.size}")
        check(self._api.visp_graph_tensor_set(self._handle, t.index, a.ctypes.data_as(c_void_p), a.nbytes))

    def get(self, t: Tensor) -> np.ndarray:
        """f32, in numpy order (reversed ne)."""
        ne = self.info(t)[1]
        out = np.empty(ne[::-1], np.float32)
        check(self._api.visp_graph_tensor_get(self._handle, t.index, out.ctypes.data_as(c_void_p), out.nbytes, 1))
        return out

    def describe(self) -> str:
        need = c_int64()
        check(self._api.visp_graph_describe(self._handle, None, 0, byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        check(self._api.visp_graph_describe(self._handle, buf, need.value, None))
        return buf.value.decode()

    def summary(self) -> dict:
        last = self.describe().strip().splitlines()[-1]
        return {k: int(v) for k, v in (kv.split("=") for kv in last.split())}


class ModelRef:
    """`visp::model_ref` (ml.h:199-245): a graph + a name prefix. `m["a"]["b"]`, `m[3]`, `m.weights("weight")`."""

    def __init__(self, graph: Graph, prefix: str = ""):
        self.graph, self.prefix = graph, prefix

    def __getitem__(self, sub) -> "ModelRef":
        sub = str(sub)
        return ModelRef(self.graph, f"{self.prefix}.{sub}" if self.prefix else sub)

    def with_prefix(self, prefix: str) -> "ModelRef":
        return ModelRef(self.graph, prefix)

    def _full(self, name: str) -> str:
        return f"{self.prefix}.{name}" if self.prefix else name

    def find(self, name: str) -> Tensor | None:
        return self.graph.find(self._full(name))

    def weights(self, name: str) -> Tensor:
        t = self.find(name)
        if t is None:
            raise KeyError(f"tensor not found: {self._full(name)}")
        return t


def named(m: ModelRef, t: Tensor) -> Tensor:  # ml.cpp:640-643
    return m.graph.set_name(t, m.prefix)


# ---- nn.h -------------------------------------------------------------------------------------------------------------------

def linear(m: ModelRef, x: Tensor) -> Tensor:  # nn.cpp:6-12
    src = [x, m.weights("weight")]
    if (b := m.find("bias")) is not None:
        src.append(b)
    return m.graph.op(OP_LINEAR, src)


def layer_norm(m: ModelRef, x: Tensor, eps: float = 1e-5) -> Tensor:  # nn.cpp:14-19
    return m.graph.op(OP_LAYER_NORM, [x, m.weights("weight"), m.weights("bias")], fparams=[eps])


def conv_2d(m: ModelRef, x: Tensor, stride: int = 1, pad: int = 0) -> Tensor:  # nn.cpp:72-100
    src = [x, m.weights("weight")]
    if (b := m.find("bias")) is not None:
        src.append(b)
    return m.graph.op(OP_CONV_2D, src, [stride, pad])


def conv_2d_depthwise(m: ModelRef, x: Tensor, stride: int = 1, pad: int = 0) -> Tensor:  # nn.cpp:102-115
    """weight [C, 1, kw, kh] (written NHWC: TinyViT's local_conv) or [1, kw, kh, C] (a depthwise OIHW kernel listed in conv2d_weights)."""
    src = [x, m.weights("weight")]
    if (b := m.find("bias")) is not None:
        src.append(b)
    return m.graph.op(OP_CONV_2D_DEPTHWISE, src, [stride, pad])


def conv_transpose_2d(m: ModelRef, x: Tensor, stride: int) -> Tensor:  # nn.cpp:117-129
    src = [x, m.weights("weight")]
    if (b := m.find("bias")) is not None:
        src.append(b)
    return m.graph.op(OP_CONV_TRANSPOSE_2D, src, [stride])


def patch_embed(m: ModelRef, x: Tensor, patch_size: int) -> Tensor:  # nn.cpp:166-180 (DINOv2: "projection", no norm; SWIN: "proj" + norm)
    p = m["proj" if m.find("proj.weight") is not None else "projection"]
    src = [x, p.weights("weight")]
    if (b := p.find("bias")) is not None:
        src.append(b)
    out = m.graph.op(OP_PATCH_EMBED, src, [patch_size])
    if m.find("norm.weight") is not None:
        out = layer_norm(m["norm"], out)
    return out


def conv_2d_deform(m: ModelRef, x: Tensor, weight: Tensor, offset: Tensor, mask: Tensor | None, stride: int, pad: int) -> Tensor:  # nn.cpp:131-148
    """weight [Cin, k, k, Cout]; offset [2 k k, OW, OH, N] (channel 2t = dy, 2t + 1 = dx of tap t); mask [k k, OW, OH, N] or None. stride 1."""
    return m.graph.op(OP_CONV_2D_DEFORM, [x, weight, offset] + ([mask] if mask is not None else []), [stride, pad])


def batch_norm_2d(m: ModelRef, x: Tensor) -> Tensor:  # nn.cpp:150-164: the statistics were folded into weight and bias at conversion
    if m.find("running_mean") is not None or m.find("running_var") is not None:
        raise ValueError("Batch norm was not fused")
    return named(m, add(m, mul(m, x, m.weights("weight")), m.weights("bias")))


def split_qkv(m: ModelRef, x: Tensor, n_heads: int, split_dim: int):  # nn.cpp:182-208
    c, n, b, _ = x.ne
    qkv = linear(m, x)
    if split_dim == 1:
        qkv = reshape(m, qkv, c // n_heads, 3, n_heads * n, b)
        qkv = cont(m, permute(m, qkv, 0, 3, 1, 2))
    elif split_dim == 2:
        qkv = reshape(m, qkv, c // n_heads, n_heads, 3, n * b)
        qkv = cont(m, permute(m, qkv, 0, 1, 3, 2))
    else:
        raise ValueError("split_qkv: split_dim is 1 or 2")
    return tuple(reshape(m, slice_(m, qkv, SLICE_ALL, SLICE_ALL, SLICE_ALL, i), c // n_heads, n_heads, n, b) for i in range(3))


def attention(m: ModelRef, q: Tensor, k: Tensor, v: Tensor, mask, scale: float, m_out: ModelRef) -> Tensor:  # nn.cpp:210-244
    """mask: None, or [n_keys, n_queries, 1 | n_heads, a divisor of batch] added to the scaled scores (head_dim 32 and 64)."""
    if mask is not None:
        x = m.graph.op(OP_ATTENTION_MASKED, [q, k, v, mask], fparams=[scale])
    else:
        x = m.graph.op(OP_ATTENTION, [q, k, v], fparams=[scale])
    return linear(m_out, x)


def attention_cross(m: ModelRef, q: Tensor, k: Tensor, v: Tensor, scale: float, m_out: ModelRef) -> Tensor:  # nn.cpp:210-244 with mask == nullptr
    """q [head_dim, n_heads, n_queries, batch], k, v [head_dim, n_heads, n_keys, batch]; head_dim 16, 32 and 64, any number of queries and keys. A builder of its own:
    attention(mask=None) keeps the head_dim-64 self-attention kernel and its refusals."""
    return linear(m_out, m.graph.op(OP_ATTENTION_CROSS, [q, k, v], fparams=[scale]))


# ---- ml.h tensor operations + the ggml ops the arch code uses directly ----------------------------------------------------------

def slice_(m: ModelRef, x: Tensor, s0=SLICE_ALL, s1=SLICE_ALL, s2=SLICE_ALL, s3=SLICE_ALL) -> Tensor:  # ml.cpp:746-768
    ip = []
    for s in (s0, s1, s2, s3):
        if isinstance(s, int):
            s = (s, s + 1, 1)
        s = tuple(s) + (1,) * (3 - len(s))
        ip += list(s)
    return m.graph.op(OP_SLICE, [x], ip)


def concat(m: ModelRef, tensors, dim: int) -> Tensor:  # ml.cpp:770-780 (n-ary: folded left to right)
    out = tensors[0]
    for t in tensors[1:]:
        out = m.graph.op(OP_CONCAT, [out, t], [dim])
    return out


def interpolate(m: ModelRef, x: Tensor, target, mode: int) -> Tensor:  # ml.cpp:782-788; x is CWHN here
    return m.graph.op(OP_INTERPOLATE, [x], [target[0], target[1], mode])


def add(m, a, b): return m.graph.op(OP_ADD, [a, b])
def mul(m, a, b): return m.graph.op(OP_MUL, [a, b])
def gelu(m, x): return m.graph.op(OP_GELU, [x])
def relu(m, x): return m.graph.op(OP_RELU, [x])
def scale(m, x, s): return m.graph.op(OP_SCALE, [x], fparams=[s])
def reshape(m, x, *ne): return m.graph.op(OP_RESHAPE, [x], list(_ne(ne)))
def repeat(m, x, *ne): return m.graph.op(OP_REPEAT, [x], list(_ne(ne)))
def cont(m, x): return m.graph.op(OP_CONT, [x])
def leaky_relu(m, x, slope): return m.graph.op(OP_LEAKY_RELU, [x], fparams=[slope])  # ggml_leaky_relu
def permute(m, x, a0, a1, a2, a3): return m.graph.op(OP_PERMUTE, [x], [a0, a1, a2, a3])  # ggml_permute: source dimension d becomes dimension a_d
def roll(m, x, s0, s1, s2, s3): return m.graph.op(OP_ROLL, [x], [s0, s1, s2, s3])  # ggml_roll
def pad(m, x, p0, p1, p2, p3): return m.graph.op(OP_PAD, [x], [p0, p1, p2, p3])  # ggml_pad
def get_rows(m, table, index): return m.graph.op(OP_GET_ROWS, [table, index])  # ggml_get_rows: a constant index is folded (f32); an i32 graph input gathers on the device (f16)
def sigmoid(m, x): return m.graph.op(OP_SIGMOID, [x])  # ggml_sigmoid
def mean_2d(m, x): return m.graph.op(OP_MEAN_2D, [x])  # birefnet.cpp:93-100: [C, W, H, N] -> [C, 1, 1, N] (not ggml_mean, which reduces ne[0])
def cast(m, x, dtype): return m.graph.op(OP_CAST, [x], [dtype])  # ggml_cast
def silu(m, x): return m.graph.op(OP_SILU, [x])  # ggml_silu
def sub(m, a, b): return m.graph.op(OP_SUB, [a, b])  # ggml_sub: a - b, b broadcast as for add
def soft_max(m, x): return m.graph.op(OP_SOFT_MAX, [x])  # ggml_soft_max: over dimension 0
def sum_rows(m, x): return m.graph.op(OP_SUM_ROWS, [x])  # ggml_sum_rows: [n, a, b, c] -> [1, a, b, c]
def clamp(m, x, lo, hi): return m.graph.op(OP_CLAMP, [x], fparams=[lo, hi])  # ggml_clamp: min(max(x, lo), hi)


def mul_mat(m, a, b): return m.graph.op(OP_MUL_MAT, [a, b])  # ggml_mul_mat: a [K, M, Ba], b [K, N, B] -> [M, N, B]
def sin(m, x): return m.graph.op(OP_SIN, [x])  # ggml_sin
def cos(m, x): return m.graph.op(OP_COS, [x])  # ggml_cos


POOL_MAX, POOL_AVG = 0, 1  # ggml_op_pool


def pool_2d(m, x, kind, k0, k1, s0, s1, p0, p1):  # ggml_pool_2d on a CWHN map
    return m.graph.op(OP_POOL_2D, [x], [kind, k0, k1, s0, s1, p0, p1])


def upscale(m, x, factor, mode):  # ggml_upscale: NEAREST is interpolate at mode 0
    return interpolate(m, x, (x.ne[1] * factor, x.ne[2] * factor), mode)


# ---- Depth-Anything-V2 against this layer (the structure of src/visp/arch/dino.cpp + depth-anything.cpp) -----------------------

BILINEAR_AC = SCALE_MODE_BILINEAR | SCALE_FLAG_ALIGN_CORNERS


def dino_interpolate_pos_encoding(m: ModelRef, x: Tensor, w: int, h: int, patch_size: int) -> Tensor:  # dino.cpp:10-30
    pos = m.weights("position_embeddings")
    n_patch, n = x.ne[1] - 1, pos.ne[1] - 1
    if n_patch == n and w == h:
        return pos
    cls_embed = slice_(m, pos, SLICE_ALL, 0)
    patch = slice_(m, pos, SLICE_ALL, (1, n + 1))
    dim = x.ne[0]
    side = int(math.sqrt(n) + 0.01)
    patch = reshape(m, patch, dim, side, side, 1)
    patch = interpolate(m, patch, (w // patch_size, h // patch_size), SCALE_MODE_BICUBIC)
    patch = reshape(m, patch, dim, (w // patch_size) * (h // patch_size), 1)
    return concat(m, [cls_embed, patch], 1)


def dino_prepare_tokens(m: ModelRef, x: Tensor, patch_size: int) -> Tensor:  # dino.cpp:32-46
    c, w, h, n = x.ne
    x = patch_embed(m["patch_embeddings"], x, patch_size)
    x = reshape(m, x, x.ne[0], x.ne[1] * x.ne[2], x.ne[3])
    cls_token = m.weights("cls_token")
    if cls_token.ne[2] != n:
        cls_token = repeat(m, cls_token, cls_token.ne[0], 1, n, 1)
    x = concat(m, [cls_token, x], 1)
    return add(m, x, dino_interpolate_pos_encoding(m, x, w, h, patch_size))


def dino_layer(m: ModelRef, x: Tensor, n_heads: int) -> Tensor:  # dino.cpp:48-90
    c, n, b, _ = x.ne
    att = layer_norm(m["norm1"], x, 1e-6)
    ma = m["attention"]
    q, k, v = (reshape(m, linear(ma["attention"][name], att), c // n_heads, n_heads, n, b) for name in ("query", "key", "value"))
    att = attention(ma, q, k, v, None, 1.0 / math.sqrt(c / n_heads), ma["output.dense"])
    x = add(m, x, mul(m, att, m["layer_scale1"].weights("lambda1")))
    ffn = layer_norm(m["norm2"], x, 1e-6)
    ffn = linear(m["mlp.fc2"], gelu(m, linear(m["mlp.fc1"], ffn)))
    x = add(m, x, mul(m, ffn, m["layer_scale2"].weights("lambda1")))
    return named(m, x)


def dino_get_intermediate_layers(m: ModelRef, x: Tensor, layers, n_layers: int, n_heads: int, patch_size: int):  # dino.cpp:92-110
    x = dino_prepare_tokens(m["embeddings"], x, patch_size)
    outputs = []
    for i in range(n_layers):
        x = dino_layer(m["encoder.layer"][i], x, n_heads)
        if i in layers:
            outputs.append(m.graph.set_name(layer_norm(m["layernorm"], x, 1e-6), f"dino_layer_{i}"))
    return outputs


def dpt_residual_conv(m: ModelRef, x: Tensor) -> Tensor:  # depth-anything.cpp:15-23
    out = conv_2d(m["convolution1"], relu(m, x), 1, 1)
    out = conv_2d(m["convolution2"], relu(m, out), 1, 1)
    return named(m, add(m, x, out))


def dpt_feature_fusion(m: ModelRef, x0: Tensor, x1: Tensor | None, size) -> Tensor:  # depth-anything.cpp:25-42
    x = x0
    if x1 is not None:
        x = add(m, x, dpt_residual_conv(m["residual_layer1"], x1))
    x = dpt_residual_conv(m["residual_layer2"], x)
    w, h = size if size is not None else (x.ne[1] * 2, x.ne[2] * 2)
    x = interpolate(m, x, (w, h), BILINEAR_AC)
    return named(m, conv_2d(m["projection"], x))


def dpt_neck(m: ModelRef, features, patch_w: int, patch_h: int) -> Tensor:  # depth-anything.cpp:44-79
    layer = []
    for i, x in enumerate(features):
        x = slice_(m, x, SLICE_ALL, (1, x.ne[1]))
        x = reshape(m, x, x.ne[0], patch_w, patch_h, x.ne[2])
        r = m["reassemble_stage.layers"][i]
        x = conv_2d(r["projection"], x)
        if i == 0:
            x = conv_transpose_2d(r["resize"], x, 4)
        elif i == 1:
            x = conv_transpose_2d(r["resize"], x, 2)
        elif i == 3:
            x = conv_2d(r["resize"], x, 2, 1)
        layer.append(x)
    layer = [conv_2d(m["convs"][i], layer[i], 1, 1) for i in range(4)]
    f = m["fusion_stage.layers"]
    fused = dpt_feature_fusion(f[0], layer[3], None, layer[2].ne[1:3])
    fused = dpt_feature_fusion(f[1], fused, layer[2], layer[1].ne[1:3])
    fused = dpt_feature_fusion(f[2], fused, layer[1], layer[0].ne[1:3])
    return dpt_feature_fusion(f[3], fused, layer[0], None)


def dpt_head(m: ModelRef, x: Tensor, w: int, h: int, max_depth: float) -> Tensor:  # depth-anything.cpp:81-96
    out = conv_2d(m["conv1"], x, 1, 1)
    out = interpolate(m, out, (w, h), BILINEAR_AC)
    out = relu(m, conv_2d(m["conv2"], out, 1, 1))
    out = relu(m, conv_2d(m["conv3"], out))
    return scale(m, out, max_depth) if max_depth != 1 else out


def depthany_predict(m: ModelRef, image: Tensor, n_layers: int, n_heads: int, patch_size: int = 14, feature_layers=(2, 5, 8, 11),
                     max_depth: float = 1.0) -> Tensor:  # depth-anything.cpp:100-110
    c, w, h, n = image.ne
    features = dino_get_intermediate_layers(m["backbone"], image, feature_layers, n_layers, n_heads, patch_size)
    fused = dpt_neck(m["neck"], features, w // patch_size, h // patch_size)
    depth = dpt_head(m["head"], fused, w, h, max_depth)
    return m.graph.output(depth, "output")


# ---- ESRGAN / Real-ESRGAN against this layer (the structure of src/visp/arch/esrgan.cpp) ---------------------------------------------------

def esrgan_upsample(m: ModelRef, x: Tensor) -> Tensor:  # esrgan.cpp:13-19
    c, w, h, n = x.ne
    x = interpolate(m, x, (w * 2, h * 2), SCALE_MODE_NEAREST)
    x = conv_2d(m, x, 1, 1)
    return named(m, leaky_relu(m, x, 0.2))


def esrgan_conv_block(m: ModelRef, x: Tensor) -> Tensor:  # esrgan.cpp:21-25
    return leaky_relu(m, conv_2d(m[0], x, 1, 1), 0.2)


def esrgan_residual_dense_block(m: ModelRef, x: Tensor) -> Tensor:  # esrgan.cpp:27-41 (channels are dimension 0 of a CWHN tensor)
    x1 = esrgan_conv_block(m["conv1"], x)
    c1 = concat(m, [x, x1], 0)
    x2 = esrgan_conv_block(m["conv2"], c1)
    c2 = concat(m, [c1, x2], 0)
    x3 = esrgan_conv_block(m["conv3"], c2)
    c3 = concat(m, [c2, x3], 0)
    x4 = esrgan_conv_block(m["conv4"], c3)
    c4 = concat(m, [c3, x4], 0)
    x5 = scale(m, conv_2d(m["conv5.0"], c4, 1, 1), 0.2)
    return named(m, add(m, x, x5))


def esrgan_rrdb(m: ModelRef, x: Tensor) -> Tensor:  # esrgan.cpp:43-51
    x_in = x
    for k in (1, 2, 3):
        x = esrgan_residual_dense_block(m[f"RDB{k}"], x)
    return named(m, add(m, scale(m, x, 0.2), x_in))


def esrgan_generate(m: ModelRef, x: Tensor, scale_factor: int, n_blocks: int) -> Tensor:  # esrgan.cpp:55-79; x = the f32 image [3, W, H, N]
    m = m["model"]
    x = conv_2d(m[0], x, 1, 1)
    sub = x
    block = m[1]["sub"]
    for i in range(n_blocks):
        sub = esrgan_rrdb(block[i], sub)
    sub = conv_2d(block[n_blocks], sub, 1, 1)
    x = add(m, x, sub)
    seq = 2
    for _ in range(int(np.log2(scale_factor))):
        x = esrgan_upsample(m[seq + 1], x)
        seq += 3
    x = leaky_relu(m, conv_2d(m[seq], x, 1, 1), 0.2)
    x = conv_2d(m[seq + 2], x, 1, 1)
    return m.graph.output(x, "result")


# ---- SWIN transformer encoder against this layer (the structure of src/visp/arch/swin.cpp) --------------------------------------------------

def swin_relative_position_index(window: int) -> np.ndarray:  # swin.cpp:26-37
    n = window
    i = np.arange(n ** 4)
    x0, y0, x1, y1 = i % n, (i // n) % n, (i // (n * n)) % n, (i // (n * n) // n) % n
    return ((y1 - y0 + n - 1) * (2 * n - 1) + (x1 - x0 + n - 1)).astype(np.int32)


def swin_attention_mask(w: int, h: int, window: int) -> np.ndarray:  # swin.cpp:165-210: [n_windows, n^2, n^2] of 0 / -inf
    n, shift = window, window // 2
    nw_x, nw_y = (w + n - 1) // n, (h + n - 1) // n
    w_pad, h_pad = nw_x * n, nw_y * n
    out = np.zeros((nw_y, nw_x, n * n, n * n), np.float32)
    y, x = np.divmod(np.arange(n * n), n)
    for iw_y in range(nw_y):
        for iw_x in range(nw_x):
            if iw_y < nw_y - 1 and iw_x < nw_x - 1:  # only the windows at the right and bottom edges carry a mask
                continue
            zone_y, zone_x = (iw_y * n + y) < h_pad - shift, (iw_x * n + x) < w_pad - shift
            match = (zone_y[:, None] == zone_y[None, :]) & (zone_x[:, None] == zone_x[None, :])
            out[iw_y, iw_x][~match] = -np.inf
    return out.reshape(nw_y * nw_x, n * n, n * n)


def swin_precompute(m: ModelRef, image_extent, window: int, n_layers: int = 4):  # swin.cpp:303-314
    """The constants the reference's caller uploads: the relative position index and one shift mask per map extent, under the names
    window_attention and layer look them up by. Called again for another extent over the same weights (BiRefNet's half-scale pass, birefnet.cpp:67-73), it
    finds the constants that exist already and adds the masks that do not."""
    g = m.graph
    width, height = image_extent[0] // 4, image_extent[1] // 4
    name = f"window_attention_{window}.rel_pos_index"
    out = [g.get_tensor(name) or g.add_weight(name, swin_relative_position_index(window), I32)]
    for i in range(n_layers + 1):
        w, h = width >> i, height >> i
        name = f"swin_layer_{w}x{h}.attn_mask"
        out.append(g.get_tensor(name) or g.add_weight(name, swin_attention_mask(w, h, window), F16))
    return out


def swin_mlp(m: ModelRef, x: Tensor) -> Tensor:  # swin.cpp:11-16
    return named(m, linear(m["fc2"], gelu(m, linear(m["fc1"], x))))


def swin_window_partition(m: ModelRef, x: Tensor, window: int) -> Tensor:  # swin.cpp:48-56
    c, w, h, b = x.ne
    assert w % window == 0 and h % window == 0, "expecting padded input"
    x = reshape(m, x, c * window, w // window, window, (h // window) * b)
    x = cont(m, permute(m, x, 0, 2, 1, 3))
    return reshape(m, x, c, window * window, (w // window) * (h // window) * b)


def swin_window_reverse(m: ModelRef, x: Tensor, w: int, h: int, window: int) -> Tensor:  # swin.cpp:58-67
    c = x.ne[0]
    b = x.ne[2] // (w // window) // (h // window)
    x = reshape(m, x, c * window, window, w // window, (h // window) * b)
    x = cont(m, permute(m, x, 0, 2, 1, 3))
    return reshape(m, x, c, w, h, b)


def swin_window_attention(m: ModelRef, x: Tensor, mask: Tensor | None, n_heads: int, window: int) -> Tensor:  # swin.cpp:69-97
    c, n, b, _ = x.ne
    rel_pos_index = m.graph.get_tensor(f"window_attention_{window}.rel_pos_index")
    rel_pos_bias = get_rows(m, m.weights("relative_position_bias_table"), rel_pos_index)
    rel_pos_bias = reshape(m, rel_pos_bias, n_heads, n, n, 1)
    rel_pos_bias = permute(m, rel_pos_bias, 2, 0, 1, 3)  # [n, n, n_heads, 1]
    rel_pos_bias = cast(m, rel_pos_bias, F16)  # get_rows gives f32
    attn_mask = rel_pos_bias
    if mask is not None:
        n_windows = mask.ne[2]
        if b > n_windows:  # several images in the batch
            mask = reshape(m, mask, n, n, n_windows, 1)
            mask = repeat(m, mask, n, n, n_windows, b // n_windows)
        mask = reshape(m, mask, n, n, 1, b)
        mask = repeat(m, mask, n, n, n_heads, b)
        attn_mask = add(m, mask, attn_mask)  # [n, n, n_heads, b] + [n, n, n_heads, 1]
    q, k, v = split_qkv(m["qkv"], x, n_heads, 2)
    x = attention(m, q, k, v, attn_mask, 1.0 / math.sqrt(c // n_heads), m["proj"])
    return named(m, x)


def swin_block(m: ModelRef, x: Tensor, mask: Tensor | None, n_heads: int, window: int, w: int, h: int, shift: int) -> Tensor:  # swin.cpp:99-141
    c, n, b, _ = x.ne
    assert n == w * h, "spatial dimensions do not match"
    shortcut = x
    x = layer_norm(m["norm1"], x)
    x = reshape(m, x, c, w, h, b)
    pad_r, pad_b = (window - w % window) % window, (window - h % window) % window
    if pad_r > 0 or pad_b > 0:
        x = pad(m, x, 0, pad_r, pad_b, 0)
    assert shift == 0 or mask is not None
    if shift > 0:
        x = roll(m, x, 0, -shift, -shift, 0)
    x = swin_window_partition(m, x, window)
    x = swin_window_attention(m["attn"], x, mask, n_heads, window)
    x = swin_window_reverse(m, x, w + pad_r, h + pad_b, window)
    if shift > 0:  # undo the shift
        x = roll(m, x, 0, shift, shift, 0)
    if pad_r > 0 or pad_b > 0:  # undo the padding
        x = reshape(m, x, c, w + pad_r, h + pad_b, b)
        x = cont(m, slice_(m, x, SLICE_ALL, (0, w), (0, h), SLICE_ALL))
    x = reshape(m, x, c, n, b)
    x = add(m, x, shortcut)
    x = add(m, x, swin_mlp(m["mlp"], layer_norm(m["norm2"], x)))
    return named(m, x)


def swin_patch_merging(m: ModelRef, x: Tensor, w: int, h: int) -> Tensor:  # swin.cpp:143-161
    c, n, b, _ = x.ne
    assert n == w * h and w % 2 == 0 and h % 2 == 0
    x = reshape(m, x, c, w, h, b)
    x = concat(m, [slice_(m, x, SLICE_ALL, (0, w, 2), (0, h, 2)), slice_(m, x, SLICE_ALL, (0, w, 2), (1, h, 2)),
                   slice_(m, x, SLICE_ALL, (1, w, 2), (0, h, 2)), slice_(m, x, SLICE_ALL, (1, w, 2), (1, h, 2))], 0)
    x = reshape(m, x, c * 4, n // 4, b)
    return named(m, linear(m["reduction"], layer_norm(m["norm"], x)))


def swin_layer(m: ModelRef, x: Tensor, w: int, h: int, depth: int, n_heads: int, window: int, down: bool):  # swin.cpp:223-244
    """Returns (x_out, w, h, x_down, w_down, h_down). The layer's mask goes to EVERY block, as the reference passes it."""
    attn_mask = m.graph.get_tensor(f"swin_layer_{w}x{h}.attn_mask")
    blocks = m["blocks"]
    for i in range(depth):
        x = swin_block(blocks[i], x, attn_mask, n_heads, window, w, h, 0 if i % 2 == 0 else window // 2)
    if down:
        return x, w, h, swin_patch_merging(m["downsample"], x, w, h), (w + 1) // 2, (h + 1) // 2
    return x, w, h, x, w, h


def swin_encode(m: ModelRef, x: Tensor, window: int, depths, n_heads):  # swin.cpp:246-266; x = the normalised f32 image [3, W, H, N]
    x = patch_embed(m["patch_embed"], x, 4)
    c, w, h, b = x.ne
    x = reshape(m, x, c, w * h, b)
    outs = []
    for i in range(len(depths)):
        x_out, w_out, h_out, x, w, h = swin_layer(m["layers"][i], x, w, h, depths[i], n_heads[i], window, i < len(depths) - 1)
        out = layer_norm(m[f"norm{i}"], x_out)
        outs.append(reshape(m, out, out.ne[0], w_out, h_out, b))
    return outs


# ---- BiRefNet decoder block against this layer (the structure of src/visp/arch/birefnet.cpp:79-145) ------------------------------------------

def birefnet_conv_2d_batch_norm(m: ModelRef, x: Tensor, stride: int = 1, pad: int = 0) -> Tensor:  # birefnet.cpp:79-81
    return conv_2d(m, x, stride, pad)  # batch_norm is fused into conv_2d at model conversion


def birefnet_deformable_conv_2d(m: ModelRef, x: Tensor, stride: int, pad: int) -> Tensor:  # birefnet.cpp:83-91
    offset = conv_2d(m["offset"], x, stride, pad)
    modulator = conv_2d(m["modulator"], x, stride, pad)
    modulator = scale(m, sigmoid(m, modulator), 2.0)
    x = conv_2d_deform(m, x, m.weights("conv.weight"), offset, modulator, stride, pad)
    return named(m, x)


def birefnet_global_avg_pool(m: ModelRef, x: Tensor) -> Tensor:  # birefnet.cpp:93-107
    x = mean_2d(m, x)
    x = relu(m, birefnet_conv_2d_batch_norm(m[1], x))
    return named(m, x)


def birefnet_aspp_module_deformable(m: ModelRef, x: Tensor, padding: int = 0) -> Tensor:  # birefnet.cpp:109-114
    x = birefnet_deformable_conv_2d(m["conv"], x, 1, padding)
    x = batch_norm_2d(m["bn"], x)
    return named(m, relu(m, x))


def birefnet_aspp_deformable(m: ModelRef, x: Tensor) -> Tensor:  # birefnet.cpp:116-137
    x1 = birefnet_aspp_module_deformable(m["aspp1"], x)
    x_deforms = [birefnet_aspp_module_deformable(m["aspp_deforms"][i], x, k // 2) for i, k in enumerate((1, 3, 7))]
    x5 = birefnet_global_avg_pool(m["global_avg_pool"], x)
    x5 = interpolate(m, x5, (x1.ne[1], x1.ne[2]), BILINEAR_AC)
    x = concat(m, [x1, *x_deforms, x5], 0)
    x = relu(m, birefnet_conv_2d_batch_norm(m["conv1"], x))
    return named(m, x)


def birefnet_basic_decoder_block(m: ModelRef, x: Tensor) -> Tensor:  # birefnet.cpp:139-145
    x = relu(m, birefnet_conv_2d_batch_norm(m["conv_in"], x, 1, 1))
    x = birefnet_aspp_deformable(m["dec_att"], x)
    x = birefnet_conv_2d_batch_norm(m["conv_out"], x, 1, 1)
    return named(m, x)


# ---- the whole BiRefNet against this layer (the structure of src/visp/arch/birefnet.cpp:20-73, 147-260) -----------------------------------------
# In CWHN: the reference's permutes to WHCN and back are views here, and its concats on dimension 2 are on dimension 0. Three departures. image_to_patches
# is one op (OP_IMAGE_PATCHES), not the reshape / permute chain, which lives in WHCN. The gate of a decoder level is mul(p, repeat(gate, p's shape)) when the
# batch is larger than 1 -- ggml_mul's broadcast written out -- since mul takes a plane [1, W, H, 1] only; with fused models either form is one pixel_gate launch.
# And encode_concat's last feature is one left fold [d0, d1, d2, xs3, up3] instead of the reference's [d0, d1, d2, concat(xs3, up3)]: the same channels
# in the same order, and one buffer that every part is written into.

def birefnet_upscale_to(m: ModelRef, x: Tensor, target: Tensor) -> Tensor:  # birefnet.cpp:20-30
    return interpolate(m, x, (target.ne[1], target.ne[2]), BILINEAR_AC)


def birefnet_downscale_by(m: ModelRef, x: Tensor, f: int) -> Tensor:  # birefnet.cpp:32-41; x an f16 map, or the f32 image
    return interpolate(m, x, (x.ne[1] // f, x.ne[2] // f), BILINEAR_AC)


def birefnet_encode_concat(m: ModelRef, xs, xs_low):  # birefnet.cpp:43-65
    ups = [birefnet_upscale_to(m, xs_low[i], xs[i]) for i in range(4)]
    out = [concat(m, [xs[i], ups[i]], 0) for i in range(3)]
    downs = [birefnet_downscale_by(m, out[i], 8 >> i) for i in range(3)]
    out.append(concat(m, [*downs, xs[3], ups[3]], 0))
    return out


def birefnet_precompute(m: ModelRef, image_extent, window: int):  # birefnet.cpp:321-323, for both passes of encode
    """The SWIN constants of the full-size and of the half-size pass (m = the model's root)."""
    swin_precompute(m["bb"], image_extent, window)
    swin_precompute(m["bb"], (image_extent[0] // 2, image_extent[1] // 2), window)


def birefnet_encode(m: ModelRef, x: Tensor, window: int, depths, n_heads):  # birefnet.cpp:67-73; x = the normalised f32 image [3, W, H, N]
    xs = swin_encode(m["bb"], x, window, depths, n_heads)
    x_low = birefnet_downscale_by(m, x, 2)
    xs_low = swin_encode(m["bb"], x_low, window, depths, n_heads)
    return birefnet_encode_concat(m, xs, xs_low)


def birefnet_simple_conv(m: ModelRef, x: Tensor) -> Tensor:  # birefnet.cpp:147-151
    x = conv_2d(m["conv1"], x, 1, 1)
    x = conv_2d(m["conv_out"], x, 1, 1)
    return named(m, x)


def birefnet_image_to_patches(m: ModelRef, x: Tensor, out_w: int, out_h: int) -> Tensor:  # birefnet.cpp:153-162; x = the f32 image -> f16 [gw gh C, out_w, out_h, N]
    return m.graph.op(OP_IMAGE_PATCHES, [x], [out_w, out_h])


def birefnet_gdt_conv(m: ModelRef, x: Tensor) -> Tensor:  # birefnet.cpp:164-168
    return relu(m, birefnet_conv_2d_batch_norm(m[0], x, 1, 1))


def birefnet_decode(m: ModelRef, x: Tensor, features, captures: bool = False) -> Tensor:  # birefnet.cpp:170-248; x = the f32 image
    g = m.graph
    x1, x2, x3, x4 = features

    def keep(t, name):
        return g.output(t, name) if captures else t

    def with_patches(blk, t):  # birefnet.cpp:181-187
        patches = birefnet_image_to_patches(m, x, t.ne[1], t.ne[2])
        patches = birefnet_simple_conv(m[blk], patches)
        return concat(m, [t, patches], 0)

    def gated(level, p):  # birefnet.cpp:189-192
        p_gdt = birefnet_gdt_conv(m[f"gdt_convs_{level}"], p)
        gdt_attn = sigmoid(m, conv_2d(m[f"gdt_convs_attn_{level}.0"], p_gdt))
        if p.ne[3] > 1:
            gdt_attn = repeat(m, gdt_attn, *p.ne)
        return mul(m, p, gdt_attn)

    p4 = keep(gated(4, birefnet_basic_decoder_block(m["block4"], with_patches("ipt_blk5", x4))), "p4")
    x3 = conv_2d(m["lateral_block4.conv"], x3)
    _p3 = add(m, birefnet_upscale_to(m, p4, x3), x3)

    p3 = keep(gated(3, birefnet_basic_decoder_block(m["block3"], with_patches("ipt_blk4", _p3))), "p3")
    _p3 = birefnet_upscale_to(m, p3, x2)
    x2 = conv_2d(m["lateral_block3.conv"], x2)
    _p2 = add(m, _p3, x2)

    p2 = keep(gated(2, birefnet_basic_decoder_block(m["block2"], with_patches("ipt_blk3", _p2))), "p2")
    _p2 = birefnet_upscale_to(m, p2, x1)
    x1 = conv_2d(m["lateral_block2.conv"], x1)
    _p1 = add(m, _p2, x1)

    _p1 = keep(birefnet_basic_decoder_block(m["block1"], with_patches("ipt_blk2", _p1)), "p1")
    _p1 = birefnet_upscale_to(m, _p1, x)
    p1_ipt = birefnet_simple_conv(m["ipt_blk1"], x)
    _p1 = concat(m, [_p1, p1_ipt], 0)
    p1_out = sigmoid(m, conv_2d(m["conv_out1.0"], _p1))
    return named(m, p1_out)


def birefnet_predict(m: ModelRef, image: Tensor, window: int, depths, n_heads, captures: bool = False) -> Tensor:  # birefnet.cpp:252-260
    """m = the model's root, after birefnet_precompute for the image's extent. captures: the encoder features, the squeeze block and the four decoder levels
    are outputs too (feature_0 .. feature_3, squeeze, p4 .. p1), as the hand schedule's captures name them."""
    g = m.graph
    features = birefnet_encode(m, image, window, depths, n_heads)
    if captures:
        features = [g.output(f, f"feature_{i}") for i, f in enumerate(features)]
    features[3] = birefnet_basic_decoder_block(m["squeeze_module.0"], features[3])
    if captures:
        g.output(features[3], "squeeze")
    scaled_preds = birefnet_decode(m["decoder"], image, features, captures)
    return g.output(scaled_preds, "output")


# ---- TinyViT (the MobileSAM image encoder) against this layer (the structure of src/visp/arch/mobile-sam.cpp:15-208) ---------------------------
# Written after the branch WITHOUT model_build_flag::window_partition (ggml_win_part is not an op here). Where it departs from the reference: the
# literal 64 of mobile-sam.cpp:195 is the last layer's resolution (a small configuration can be built), the two GGML_ASSERTs of tiny_vit_block are
# exceptions, window_reverse takes the batch from the window count (the reference reads ne[3] of a 3-D tensor: batch 1 only), and patch_merging
# reads its width from conv1's output instead of from dimension 0 of the depthwise kernel (which is 1 in the [1, kw, kh, C] form).

def sam_conv_2d_batch_norm(m: ModelRef, x: Tensor, stride: int = 1, pad: int = 0) -> Tensor:  # mobile-sam.cpp:15-18
    return conv_2d(m["c"], x, stride, pad)  # batch_norm is fused into conv_2d at model conversion


def sam_conv_2d_depthwise_batch_norm(m: ModelRef, x: Tensor, stride: int = 1, pad: int = 0) -> Tensor:  # mobile-sam.cpp:20-23
    return conv_2d_depthwise(m["c"], x, stride, pad)


def sam_window_partition(m: ModelRef, x: Tensor, window: int) -> Tensor:  # mobile-sam.cpp:25-44
    c, w, h, b = x.ne
    px, py = (window - w % window) % window, (window - h % window) % window
    npw, nph = (w + px) // window, (h + py) // window
    if px > 0 or py > 0:
        x = pad(m, x, 0, px, py, 0)
    x = reshape(m, x, c * window, npw, window, nph * b)
    x = cont(m, permute(m, x, 0, 2, 1, 3))
    return reshape(m, x, c, window * window, npw * nph * b)


def sam_window_reverse(m: ModelRef, x: Tensor, w: int, h: int, window: int) -> Tensor:  # mobile-sam.cpp:46-65
    c = x.ne[0]
    px, py = (window - w % window) % window, (window - h % window) % window
    npw, nph = (w + px) // window, (h + py) // window
    b = x.ne[2] // (npw * nph)
    x = reshape(m, x, c * window, window, npw, nph * b)
    x = cont(m, permute(m, x, 0, 2, 1, 3))
    x = reshape(m, x, c, w + px, h + py, b)
    x = slice_(m, x, SLICE_ALL, (0, w), (0, h))
    return cont(m, x)


def tinyvit_patch_embed(m: ModelRef, x: Tensor) -> Tensor:  # mobile-sam.cpp:71-76; x = the normalised f32 image [3, W, H, N]
    x = sam_conv_2d_batch_norm(m["seq.0"], x, 2, 1)
    x = gelu(m, x)
    x = sam_conv_2d_batch_norm(m["seq.2"], x, 2, 1)
    return named(m, x)


def tinyvit_mb_conv(m: ModelRef, x: Tensor) -> Tensor:  # mobile-sam.cpp:78-92
    shortcut = x
    x = gelu(m, sam_conv_2d_batch_norm(m["conv1"], x))
    x = gelu(m, sam_conv_2d_depthwise_batch_norm(m["conv2"], x, 1, 1))
    x = sam_conv_2d_batch_norm(m["conv3"], x)
    x = gelu(m, add(m, x, shortcut))
    return named(m, x)


def tinyvit_patch_merging(m: ModelRef, x: Tensor) -> Tensor:  # mobile-sam.cpp:94-113
    x = gelu(m, sam_conv_2d_batch_norm(m["conv1"], x))
    c_out = x.ne[0]
    stride = 1 if c_out in (320, 448, 576) else 2
    x = gelu(m, sam_conv_2d_depthwise_batch_norm(m["conv2"], x, stride, 1))
    c, w, h, b = x.ne
    x = sam_conv_2d_batch_norm(m["conv3"], x)
    return named(m, reshape(m, x, c, w * h, b))  # always [c, wh, b]


def tinyvit_mlp(m: ModelRef, x: Tensor) -> Tensor:  # mobile-sam.cpp:115-122
    x = layer_norm(m["norm"], x)
    x = gelu(m, linear(m["fc1"], x))
    return named(m, linear(m["fc2"], x))


def tinyvit_attention_rel_bias(m: ModelRef, x: Tensor, dim: int, n_heads: int) -> Tensor:  # mobile-sam.cpp:124-132
    scale_ = 1.0 / math.sqrt(float(dim // n_heads))
    mask = m.weights("attention_biases_indexed")  # [T, T, heads, 1]
    x = layer_norm(m["norm"], x)
    q, k, v = split_qkv(m["qkv"], x, n_heads, 1)
    return attention(m, q, k, v, mask, scale_, m["proj"])


def tinyvit_block(m: ModelRef, x: Tensor, input_resolution: int, dim: int, num_heads: int, window_size: int) -> Tensor:  # mobile-sam.cpp:134-161
    h = w = input_resolution
    c, spatial, b, _ = x.ne
    if spatial != h * w:
        raise ValueError(f"tinyvit_block: {spatial} tokens do not form a {w}x{h} map")
    if h == window_size or w == window_size:
        raise ValueError(f"tinyvit_block: a {w}x{h} map that is one {window_size}x{window_size} window is not built (the reference asserts the same)")
    res_x = x
    x = reshape(m, x, c, w, h, b)
    x = sam_window_partition(m, x, window_size)
    x = tinyvit_attention_rel_bias(m["attn"], x, dim, num_heads)
    x = sam_window_reverse(m, x, w, h, window_size)
    x = reshape(m, x, c, spatial, b)
    x = add(m, x, res_x)
    x = reshape(m, x, c, w, h, b)
    x = sam_conv_2d_depthwise_batch_norm(m["local_conv"], x, 1, 1)  # (its kernel is stored NHWC whatever the file's layout: [C, 1, kw, kh])
    x = reshape(m, x, c, spatial, b)
    x = add(m, x, tinyvit_mlp(m["mlp"], x))
    return named(m, x)


def tinyvit_conv_layer(m: ModelRef, x: Tensor, layer) -> Tensor:  # mobile-sam.cpp:163-170; layer = (resolution, dim, depth, heads, window, downsample)
    for i in range(layer[2]):
        x = tinyvit_mb_conv(m["blocks"][i], x)
    x = tinyvit_patch_merging(m["downsample"], x)
    return named(m, x)


def tinyvit_basic_layer(m: ModelRef, x: Tensor, layer) -> Tensor:  # mobile-sam.cpp:172-183
    resolution, dim, depth, heads, window, downsample = layer
    for i in range(depth):
        x = tinyvit_block(m["blocks"][i], x, resolution, dim, heads, window)
    if downsample:
        x = reshape(m, x, x.ne[0], resolution, resolution, x.ne[2])
        x = tinyvit_patch_merging(m["downsample"], x)
    return named(m, x)


def tinyvit_encode(m: ModelRef, x: Tensor, layers) -> Tensor:  # mobile-sam.cpp:185-208; layers as synth.TinyVitConfig.layers() gives them
    x = tinyvit_patch_embed(m["patch_embed"], x)
    x = tinyvit_conv_layer(m["layers.0"], x, layers[0])
    for i in range(1, len(layers)):
        x = tinyvit_basic_layer(m["layers"][i], x, layers[i])
    res = layers[-1][0]
    x = reshape(m, x, x.ne[0], res, res, x.ne[2])
    x = conv_2d(m["neck.0"], x)
    x = layer_norm(m["neck.1"], x)
    x = conv_2d(m["neck.2"], x, 1, 1)
    return layer_norm(m["neck.3"], x)


# ---- YOLOv9t against this layer (the structure of src/visp/arch/yolov9t.cpp) ------------------------------------------------------------------
# Node for node, with `m` the model's root and tensor names as the reference builds them (BatchNorm is folded into the conv at conversion, so Conv's
# batch_norm_2d branch has nothing to do). Four departures, because the reference's detect head holds for one image only:
# reshape_2d keeps the batch ([C, w h, 1, N]); ggml_view_4d / ggml_dup are channel slices; sub(anchor_points, lt) is add(scale(lt, -1), anchors), since a
# constant cannot be the larger operand; and the stride constant is [4, A] made on the host, since mul does not broadcast along dimension 0.

YOLO_REG_MAX = 16


def _yolo_at(m: ModelRef, name: str) -> ModelRef:
    return m.with_prefix(m._full(name))


def yolo_conv(m: ModelRef, x: Tensor, name: str, k: int, s: int = 1, act: bool = True) -> Tensor:  # yolov9t.cpp:78-130
    """Conv: conv_2d at autopad k // 2 under `name` (".conv" appended when it is missing), then SiLU."""
    x = conv_2d(_yolo_at(m, name if ".conv" in name else name + ".conv"), x, s, k // 2)
    return silu(m, x) if act else x


def yolo_aconv(m: ModelRef, x: Tensor, name: str) -> Tensor:  # yolov9t.cpp:165-185
    pooled = pool_2d(m, x, POOL_AVG, 2, 2, 1, 1, 0, 0)
    return yolo_conv(m, pooled, name + ".cv1.conv", 3, 2)


def yolo_concat(m: ModelRef, tensors, dim: int = 0) -> Tensor:  # yolov9t.cpp:495-503 and yolo_concat: channels are dimension 0 of a CWHN map
    return concat(m, list(tensors), dim)


def yolo_upsample(m: ModelRef, x: Tensor, scale_factor: int = 2) -> Tensor:  # yolov9t.cpp:486-493
    return upscale(m, x, scale_factor, SCALE_MODE_NEAREST)


def yolo_elan1(m: ModelRef, x: Tensor, name: str, c1: int, c2: int, c3: int, c4: int) -> Tensor:  # yolov9t.cpp:187-234
    assert c3 % 2 == 0, "ELAN1: c3 must be even for chunk(2)"
    cv1 = yolo_conv(m, x, name + ".cv1.conv", 1)
    split1 = slice_(m, cv1, (0, c3 // 2))
    split2 = slice_(m, cv1, (c3 // 2, c3))
    cv2 = yolo_conv(m, split2, name + ".cv2.conv", 3)
    cv3 = yolo_conv(m, cv2, name + ".cv3.conv", 3)
    cat = yolo_concat(m, [yolo_concat(m, [yolo_concat(m, [split1, split2]), cv2]), cv3])
    return yolo_conv(m, cat, name + ".cv4.conv", 1)


def yolo_rep_conv(m: ModelRef, x: Tensor, name: str, s: int = 1, act: bool = True) -> Tensor:  # yolov9t.cpp:256-300, the non-deploy branch (k = 3, p = 1)
    out = add(m, yolo_conv(m, x, name + ".conv1.conv", 3, s, False), yolo_conv(m, x, name + ".conv2.conv", 1, s, False))
    return silu(m, out) if act else out


def yolo_rep_bottleneck(m: ModelRef, x: Tensor, name: str, c1: int, c2: int, shortcut: bool = True) -> Tensor:  # yolov9t.cpp:304-332
    cv2 = yolo_conv(m, yolo_rep_conv(m, x, name + ".cv1"), name + ".cv2", 3)
    return add(m, x, cv2) if shortcut and c1 == c2 else cv2


def yolo_rep_csp(m: ModelRef, x: Tensor, name: str, c1: int, c2: int, n: int, shortcut: bool = True, e: float = 0.5) -> Tensor:  # yolov9t.cpp:370-402
    c_ = int(c2 * e)
    cv1 = yolo_conv(m, x, name + ".cv1", 1)
    cv2 = yolo_conv(m, x, name + ".cv2", 1)
    m_out = cv1
    for i in range(n):
        m_out = yolo_rep_bottleneck(m, m_out, f"{name}.m.{i}", c_, c_, shortcut)
    return yolo_conv(m, cont(m, concat(m, [m_out, cv2], 0)), name + ".cv3", 1)


def yolo_rep_ncsp_elan4(m: ModelRef, x: Tensor, name: str, c1: int, c2: int, c3: int, c4: int, n: int) -> Tensor:  # yolov9t.cpp:406-445
    c = c3 // 2
    cv1 = yolo_conv(m, x, name + ".cv1", 1)
    h0 = slice_(m, cv1, (0, c))
    h1 = slice_(m, cv1, (c, c3))

    def rep_conv(x, name, c_in, c_out):
        return yolo_conv(m, yolo_rep_csp(m, x, name + ".0", c_in, c_out, n), name + ".1", 3)

    cv2 = rep_conv(h1, name + ".cv2", c3 // 2, c4)
    cv3 = rep_conv(cv2, name + ".cv3", c4, c4)
    return yolo_conv(m, yolo_concat(m, [h0, h1, cv2, cv3]), name + ".cv4", 1)


def yolo_sppelan(m: ModelRef, x: Tensor, name: str, c1: int, c2: int, c3: int, k: int = 5) -> Tensor:  # yolov9t.cpp:449-483
    cv1 = yolo_conv(m, x, name + ".cv1", 1)
    cv2 = pool_2d(m, cv1, POOL_MAX, k, k, 1, 1, k // 2, k // 2)
    cv3 = pool_2d(m, cv2, POOL_MAX, k, k, 1, 1, k // 2, k // 2)
    cv4 = pool_2d(m, cv3, POOL_MAX, k, k, 1, 1, k // 2, k // 2)
    return yolo_conv(m, cont(m, yolo_concat(m, [cv1, cv2, cv3, cv4])), name + ".cv5", 1)


def yolov9t_backbone(m: ModelRef, x: Tensor) -> dict[int, Tensor]:  # yolov9t.cpp:507-628; x = the f32 image [3, S, S, N]
    f: dict[int, Tensor] = {}
    f[0] = yolo_conv(m, x, "model.0", 3, 2)
    f[1] = yolo_conv(m, f[0], "model.1", 3, 2)
    f[2] = yolo_elan1(m, f[1], "model.2", 32, 32, 32, 16)
    f[3] = yolo_aconv(m, f[2], "model.3")
    f[4] = yolo_rep_ncsp_elan4(m, f[3], "model.4", 64, 64, 64, 32, 3)
    f[5] = yolo_aconv(m, f[4], "model.5")
    f[6] = yolo_rep_ncsp_elan4(m, f[5], "model.6", 96, 96, 96, 48, 3)
    f[7] = yolo_aconv(m, f[6], "model.7")
    f[8] = yolo_rep_ncsp_elan4(m, f[7], "model.8", 128, 128, 128, 64, 3)
    f[9] = yolo_sppelan(m, f[8], "model.9", 128, 128, 64, 5)
    f[10] = yolo_upsample(m, f[9], 2)
    f[11] = yolo_concat(m, [f[10], f[6]])
    f[12] = yolo_rep_ncsp_elan4(m, f[11], "model.12", 224, 96, 96, 48, 3)
    f[13] = yolo_upsample(m, f[12], 2)
    f[14] = yolo_concat(m, [f[13], f[4]])
    f[15] = yolo_rep_ncsp_elan4(m, f[14], "model.15", 160, 64, 64, 32, 3)
    f[16] = yolo_aconv(m, f[15], "model.16")
    f[17] = yolo_concat(m, [f[16], f[12]])
    f[18] = yolo_rep_ncsp_elan4(m, f[17], "model.18", 144, 96, 96, 48, 3)
    f[19] = yolo_aconv(m, f[18], "model.19")
    f[20] = yolo_concat(m, [f[19], f[9]])
    f[21] = yolo_rep_ncsp_elan4(m, f[20], "model.21", 192, 128, 128, 64, 3)
    return f


def yolo_dist2bbox(m: ModelRef, distance: Tensor, anchor_points: Tensor) -> Tensor:  # yolov9t.cpp:631-655, xyxy; distance [1, 4, A, N], anchors [2, A]
    distance = cont(m, permute(m, cont(m, distance), 2, 0, 1, 3))  # [4, A, 1, N]
    lt = slice_(m, distance, (0, 2))
    rb = slice_(m, distance, (2, 4))
    x1y1 = add(m, scale(m, lt, -1.0), anchor_points)  # anchor_points - lt
    x2y2 = add(m, rb, anchor_points)
    return concat(m, [x1y1, x2y2], 0)


def yolo_dfl_forward(m: ModelRef, proj: Tensor, x: Tensor, reg_max: int) -> Tensor:  # yolov9t.cpp:657-691; x [4 reg_max, A, 1, N] -> [1, 4, A, N]
    anchors, batch = x.ne[1] * x.ne[2], x.ne[3]
    soft = soft_max(m, reshape(m, cont(m, x), reg_max, 4, anchors, batch))
    return sum_rows(m, mul(m, soft, reshape(m, proj, reg_max, 1, 1, 1)))


def yolo_make_anchors(levels, strides, offset: float = 0.5):  # yolov9t.cpp:875-925: (x + 0.5, y + 0.5) y-major per level, and each anchor's stride
    pts, st = [], []
    for (w, h), s in zip(levels, strides):
        gy, gx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        pts.append(np.stack([gx.ravel() + offset, gy.ravel() + offset], -1))
        st.append(np.full(w * h, s))
    return np.concatenate(pts).astype(np.float32), np.concatenate(st).astype(np.float32)


def yolo_inference(m: ModelRef, raw, features, reg_max: int, nc: int):  # yolov9t.cpp:693-768 -> boxes [4, A, 1, N], scores [nc, A, 1, N]
    g = m.graph
    x_cat = yolo_concat(m, features, 1)  # [4 reg_max + nc, A, 1, N]
    total = x_cat.ne[1]
    anchors, strides = yolo_make_anchors([(r.ne[1], r.ne[2]) for r in raw], [8.0 * 2 ** i for i in range(len(raw))])
    tag = "x".join(str(r.ne[1]) for r in raw)
    anchor_points = g.get_tensor(f"anchor_points_{tag}") or g.add_weight(f"anchor_points_{tag}", anchors, F32)
    stride_tensor = g.get_tensor(f"stride_points_{tag}") or g.add_weight(f"stride_points_{tag}", np.repeat(strides[:, None], 4, 1), F32)  # [4, A]
    box = cont(m, slice_(m, x_cat, (0, reg_max * 4)))
    cls = cont(m, slice_(m, x_cat, (reg_max * 4, reg_max * 4 + nc)))
    proj = g.get_tensor("dfl_proj") or g.add_weight("dfl_proj", np.arange(reg_max, dtype=np.float32), F32)
    dbox = yolo_dist2bbox(m, yolo_dfl_forward(m, proj, box, reg_max), anchor_points)
    dbox = mul(m, dbox, stride_tensor)
    assert dbox.ne[1] == total
    return dbox, g.set_name(sigmoid(m, cls), "cls_prob")


def yolo_detect_forward(m: ModelRef, features, ch, nc: int, training: bool = False):  # yolov9t.cpp:770-824
    """-> (boxes, scores, raw maps); boxes and scores are None when `training` (the convs alone)."""
    reg_max = YOLO_REG_MAX
    raw, flat = [], []
    for i, x in enumerate(features):
        r = yolo_conv(m, yolo_conv(m, x, f"detect.cv2.{i}.0.conv", 3), f"detect.cv2.{i}.1.conv", 3)
        r = conv_2d(_yolo_at(m, f"detect.cv2.{i}.2"), r, 1, 0)
        c = yolo_conv(m, yolo_conv(m, x, f"detect.cv3.{i}.0.conv", 3), f"detect.cv3.{i}.1.conv", 3)
        c = conv_2d(_yolo_at(m, f"detect.cv3.{i}.2"), c, 1, 0)
        combined = yolo_concat(m, [r, c])
        raw.append(combined)
        flat.append(reshape(m, combined, combined.ne[0], combined.ne[1] * combined.ne[2], 1, combined.ne[3]))
    if training:
        return None, None, raw
    boxes, scores = yolo_inference(m, raw, flat, reg_max, nc)
    return boxes, scores, raw


def yolov9t_forward(m: ModelRef, image: Tensor, nc: int = 80):  # yolov9t.cpp:827-840; image f32 [3, S, S, N]
    """-> (boxes [4, A, 1, N] xyxy in pixels, scores [nc, A, 1, N], the per-level raw maps [64 + nc, S / s, S / s, N], the backbone's features by index)."""
    f = yolov9t_backbone(m, image)
    boxes, scores, raw = yolo_detect_forward(m, [f[15], f[18], f[21]], [64, 96, 128], nc)
    return boxes, scores, raw, f


# ---- MI-GAN against this layer (the structure of src/visp/arch/migan.cpp, its CWHN branch) ------------------------------------------------------
# Node for node. One departure, in the manner of the four of the YOLO builders: the image path (torgb, upsample_2d(img), add) has 3
# channels and every map kernel here works on multiples of 8, so torgb's weight and bias and the image upsample's filter enter as named host constants 8
# channels wide, channels 3..7 exactly zero; the image is carried 8 wide and migan_generate ends with a channel slice 0..3.

MIGAN_SQRT2 = 1.4142135623  # migan.cpp:15


def _migan_pad8(m: ModelRef, name: str, axis: int) -> Tensor:
    """The constant `name` under m with numpy axis `axis` (the channel) zero-padded from 3 to 8, as the named host constant '<name>.pad8'."""
    g, full = m.graph, m._full(name) + ".pad8"
    if (t := g.get_tensor(full)) is not None:
        return t
    a = g.read_constant(m.weights(name))
    width = [(0, 0)] * a.ndim
    width[axis] = (0, 8 - a.shape[axis])
    return g.add_weight(full, np.pad(a, width), F16)


def migan_lrelu_agc(m: ModelRef, x: Tensor, alpha: float, gain: float, clamp_: float) -> Tensor:  # migan.cpp:17-26
    x = leaky_relu(m, x, alpha)
    if gain != 1:
        x = scale(m, x, gain)
    if clamp_ != 0:
        x = clamp(m, x, -clamp_, clamp_)
    return named(m, x)


def migan_downsample_2d(m: ModelRef, x: Tensor) -> Tensor:  # migan.cpp:28-30
    return conv_2d_depthwise(m["filter"], x, 2, 1)


def migan_upsample_2d(m: ModelRef, x: Tensor, fir: Tensor | None = None) -> Tensor:  # migan.cpp:32-51; `fir`: the 4x4 kernel, where it is not m["filter"]'s weight
    filt = m.weights("filter_const")
    filt = reshape(m, filt, 1, filt.ne[0], filt.ne[1], 1)
    c, w, h, n = x.ne
    x = interpolate(m, x, (w * 2, h * 2), SCALE_MODE_NEAREST)
    x = mul(m, x, filt)
    x = conv_2d_depthwise(m["filter"], x, 1, 2) if fir is None else m.graph.op(OP_CONV_2D_DEPTHWISE, [x, fir], [1, 2])  # 4x4 filter
    x = slice_(m, x, SLICE_ALL, (0, -1), (0, -1), SLICE_ALL)  # remove padding from right and bottom
    x = cont(m, x)
    return named(m, x)


def migan_separable_conv_2d(m: ModelRef, x: Tensor, activation: bool = False, downsample: bool = False, upsample: bool = False, noise: bool = False) -> Tensor:  # migan.cpp:53-82
    pad_ = m["conv1"].weights("weight").ne[2] // 2
    x = conv_2d_depthwise(m["conv1"], x, 1, pad_)
    if activation:
        x = migan_lrelu_agc(m, x, 0.2, MIGAN_SQRT2, 256)
    if downsample:
        x = migan_downsample_2d(m["downsample"], x)
    x = conv_2d(m["conv2"], x)
    if upsample:
        x = migan_upsample_2d(m["upsample"], x)
    if noise:
        nz = mul(m, m.weights("noise_const"), m.weights("noise_strength"))
        nz = reshape(m, nz, 1, nz.ne[0], nz.ne[1], 1)
        x = add(m, x, nz)
    if activation:
        x = migan_lrelu_agc(m, x, 0.2, MIGAN_SQRT2, 256)
    return named(m, x)


def migan_from_rgb(m: ModelRef, x: Tensor) -> Tensor:  # migan.cpp:84-89; x = the f32 image [4, W, H, N]
    x = conv_2d(m["fromrgb"], x)
    x = migan_lrelu_agc(m, x, 0.2, MIGAN_SQRT2, 256)
    return named(m, x)


def migan_encoder_block(m: ModelRef, x: Tensor, downsample: bool = False):  # migan.cpp:91-95
    feat = migan_separable_conv_2d(m["conv1"], x, activation=True)
    x = migan_separable_conv_2d(m["conv2"], feat, activation=True, downsample=downsample)
    return x, feat


def migan_encode(m: ModelRef, x: Tensor, res: int):  # migan.cpp:99-112
    assert res == x.ne[1]
    n = int(math.log2(res)) - 1
    assert (1 << (n + 1)) == res
    x = migan_from_rgb(m[f"b{res}"], x)
    feats = [None] * n
    for i in range(n - 1):
        x, feats[i] = migan_encoder_block(m[f"b{res >> i}"], x, downsample=True)
    x, feats[n - 1] = migan_encoder_block(m["b4"], x)
    return x, feats


def migan_synthesis_block(m: ModelRef, x: Tensor, feat: Tensor, img: Tensor | None, upsample: bool = False, noise: bool = False):  # migan.cpp:114-127
    """`img` and the returned image are 8 channels wide, channels 3..7 zero (the departure above)."""
    x = migan_separable_conv_2d(m["conv1"], x, activation=True, noise=noise, upsample=upsample)
    x = add(m, x, feat)
    x = migan_separable_conv_2d(m["conv2"], x, activation=True, noise=noise)
    if img is not None:
        img = migan_upsample_2d(m["upsample"], img, _migan_pad8(m["upsample.filter"], "weight", 0))
    y = m.graph.op(OP_CONV_2D, [x, _migan_pad8(m["torgb"], "weight", 0), _migan_pad8(m["torgb"], "bias", -1)], [1, 0])
    img = add(m, img, y) if img is not None else y
    return x, img


def migan_synthesis(m: ModelRef, x: Tensor, feats, res: int) -> Tensor:  # migan.cpp:129-140
    n = int(math.log2(res)) - 1
    assert (1 << (n + 1)) == res
    x, img = migan_synthesis_block(m["b4"], x, feats[n - 1], None)
    for i in range(n - 2, -1, -1):
        x, img = migan_synthesis_block(m[f"b{res >> i}"], x, feats[i], img, upsample=True, noise=True)
    return img


def migan_generate(m: ModelRef, image: Tensor, res: int) -> Tensor:  # migan.cpp:161-165; image f32 [4, res, res, N] -> f16 [3, res, res, N]
    x, feats = migan_encode(m["encoder"], image, res)
    img = migan_synthesis(m["synthesis"], x, feats, res)
    return m.graph.output(slice_(m, img, (0, 3)), "output")


# ---- MobileSAM prompt encoder and mask decoder against this layer (the structure of src/visp/arch/mobile-sam.cpp:210-478) ------------------------------
# Node for node, with three departures. The reference writes into views (ggml_cpy into a slice, :256 and :468; ggml_add_inplace on a slice, :261, :275, :279);
# this layer is functional, so those are concat(add(slice(..), w), ..) and a concat of the four hypernetwork rows. attention() with a null mask is
# attention_cross(): the builder of the op that takes any head_dim in {16, 32, 64} and T_q != T_k. And pos_src is repeated to the batch of the tokens (the
# reference repeats it to tokens->ne[3], which is 1, and its reshape_3d to b then holds for one prompt only); several prompts are batch entries here.

def sam_position_embedding_random(m: ModelRef, coords: Tensor) -> Tensor:  # mobile-sam.cpp:238-248; coords f32 [2, n, B] in [-1, 1]
    pe = m.weights("positional_encoding_gaussian_matrix")  # [F, 2]
    pe = cont(m, permute(m, pe, 1, 0, 2, 3))  # ggml_transpose
    coords = mul_mat(m, pe, coords)
    coords = scale(m, coords, 2.0 * math.pi)
    return concat(m, [sin(m, coords), cos(m, coords)], 0)


def sam_embed_points(m: ModelRef, coords: Tensor) -> Tensor:  # mobile-sam.cpp:250-266; the last point is the sentinel
    count, b = coords.ne[1] - 1, coords.ne[2]
    x = sam_position_embedding_random(m["pe_layer"], coords)
    c = x.ne[0]
    label_end = repeat(m, m.weights("not_a_point_embed.weight"), c, 1, b, 1)  # :255-256: the sentinel's row IS not_a_point_embed
    label_one = add(m, slice_(m, x, SLICE_ALL, (0, count)), m.weights("point_embeddings.1.weight"))  # :260-261: foreground points
    return concat(m, [label_one, label_end], 1)


def sam_embed_box(m: ModelRef, coords: Tensor) -> Tensor:  # mobile-sam.cpp:268-284; coords f32 [2, 2, B]: the two corners
    x = sam_position_embedding_random(m["pe_layer"], coords)
    corner1 = add(m, slice_(m, x, SLICE_ALL, 0), m.weights("point_embeddings.2.weight"))
    corner2 = add(m, slice_(m, x, SLICE_ALL, 1), m.weights("point_embeddings.3.weight"))
    return m.graph.set_name(concat(m, [corner1, corner2], 1), "box_embed")


def sam_no_mask_embed(m: ModelRef) -> Tensor:  # mobile-sam.cpp:286-288
    return m.weights("no_mask_embed.weight")


def sam_mlp_block(m: ModelRef, x: Tensor) -> Tensor:  # mobile-sam.cpp:294-299
    return linear(m["lin2"], relu(m, linear(m["lin1"], x)))


def sam_decoder_attention(m: ModelRef, q: Tensor, k: Tensor, v: Tensor, n_heads: int) -> Tensor:  # mobile-sam.cpp:307-319
    q, k, v = linear(m["q_proj"], q), linear(m["k_proj"], k), linear(m["v_proj"], v)
    q, k, v = (reshape(m, t, t.ne[0] // n_heads, n_heads, t.ne[1], t.ne[2]) for t in (q, k, v))
    return attention_cross(m, q, k, v, 1.0 / math.sqrt(float(q.ne[0])), m["out_proj"])


def sam_two_way_attention_block(m: ModelRef, queries: Tensor, keys: Tensor, query_pe: Tensor, key_pe: Tensor, num_heads: int, skip_first_layer_pe: bool):  # mobile-sam.cpp:321-362
    if skip_first_layer_pe:  # self attention block
        queries = sam_decoder_attention(m["self_attn"], queries, queries, queries, num_heads)
    else:
        q = add(m, queries, query_pe)
        queries = add(m, queries, sam_decoder_attention(m["self_attn"], q, q, queries, num_heads))
    queries = layer_norm(m["norm1"], queries)
    q = add(m, queries, query_pe)  # cross attention block, tokens attending to image embedding
    k = add(m, keys, key_pe)
    queries = add(m, queries, sam_decoder_attention(m["cross_attn_t2i"], q, k, keys, num_heads))
    queries = layer_norm(m["norm2"], queries)
    queries = add(m, queries, sam_mlp_block(m["mlp"], queries))  # MLP block
    queries = cont(m, layer_norm(m["norm3"], queries))
    q = add(m, queries, query_pe)  # cross attention block, image embedding attending to tokens
    keys = add(m, keys, sam_decoder_attention(m["cross_attn_i2t"], k, q, queries, num_heads))
    keys = layer_norm(m["norm4"], keys)
    return queries, keys


def sam_two_way_transformer(m: ModelRef, image_embedding: Tensor, image_pe: Tensor, point_embedding: Tensor, depth: int, num_heads: int):  # mobile-sam.cpp:364-395
    c, w, h, b = image_embedding.ne
    image_embedding = reshape(m, image_embedding, c, w * h, b)
    image_pe = reshape(m, image_pe, c, w * h, b)
    queries, keys = point_embedding, image_embedding
    for i in range(depth):
        queries, keys = sam_two_way_attention_block(m["layers"][i], queries, keys, point_embedding, image_pe, num_heads, i == 0)
    q = add(m, queries, point_embedding)  # the final attention layer from the points to the image
    k = add(m, keys, image_pe)
    queries = add(m, queries, sam_decoder_attention(m["final_attn_t2i"], q, k, keys, num_heads))
    return layer_norm(m["norm_final_attn"], queries), keys


def sam_upscale_outputs(m: ModelRef, x: Tensor) -> Tensor:  # mobile-sam.cpp:397-405
    x = conv_transpose_2d(m[0], x, 2)
    x = gelu(m, layer_norm(m[1], x))
    return gelu(m, conv_transpose_2d(m[3], x, 2))


def sam_hypernetwork_mlp(m: ModelRef, x: Tensor, num_layers: int) -> Tensor:  # mobile-sam.cpp:407-416
    for i in range(num_layers):
        x = linear(m["layers"][i], x)
        if i < num_layers - 1:
            x = relu(m, x)
    return x


def sam_predict_masks(m: ModelRef, image_embeddings: Tensor, sparse_prompt: Tensor, dense_prompt: Tensor):  # mobile-sam.cpp:418-478
    """image_embeddings [C, W, H, 1], sparse_prompt [C, n, B] (B prompts), dense_prompt [C] -> masks [4 W, 4 H, 4, B], iou [4, B]."""
    num_heads, transformer_depth, num_mask_tokens = 8, 2, 4
    b = sparse_prompt.ne[2]
    output_tokens = concat(m, [m.weights("iou_token.weight"), m.weights("mask_tokens.weight")], 1)
    output_tokens = repeat(m, output_tokens, output_tokens.ne[0], output_tokens.ne[1], b, 1)
    tokens = concat(m, [output_tokens, sparse_prompt], 1)
    ie0, ie1, ie2, _ = image_embeddings.ne
    src = repeat(m, image_embeddings, ie0, ie1, ie2, b)  # per-image data in batch direction to be per-mask
    src = add(m, src, dense_prompt)
    image_pe = m.weights("dense_positional_embedding")
    pos_src = repeat(m, image_pe, image_pe.ne[0], image_pe.ne[1], image_pe.ne[2], b)
    c_low, w_low, h_low, _ = src.ne
    hs, out = sam_two_way_transformer(m["transformer"], src, pos_src, tokens, transformer_depth, num_heads)
    iou_token_out = reshape(m, slice_(m, hs, SLICE_ALL, 0), hs.ne[0], b)  # ggml_view_2d(hs, ne0, ne2, nb2, 0): token 0 of every prompt
    mask_tokens_out = slice_(m, hs, SLICE_ALL, (1, num_mask_tokens + 1))
    out = reshape(m, out, c_low, w_low, h_low, b)
    upscaled_embedding = sam_upscale_outputs(m["output_upscaling"], out)
    c, w, h, _ = upscaled_embedding.ne
    upscaled_embedding = reshape(m, upscaled_embedding, c, w * h, b)
    mlps = m["output_hypernetworks_mlps"]
    rows = [sam_hypernetwork_mlp(mlps[i], slice_(m, mask_tokens_out, SLICE_ALL, i), 3) for i in range(num_mask_tokens)]
    hyper_in = concat(m, rows, 1)  # :462-470 writes the rows into a new tensor
    masks = mul_mat(m, upscaled_embedding, hyper_in)
    masks = reshape(m, masks, w, h, masks.ne[1], b)
    iou_pred = sam_hypernetwork_mlp(m["iou_prediction_head"], iou_token_out, 3)
    return masks, iou_pred


def sam_predict_mask(m: ModelRef, image_embed: Tensor, prompt_embed: Tensor):  # mobile-sam.cpp:597-602; m = the model's root
    dense_prompt = sam_no_mask_embed(m["prompt_encoder"])
    masks, iou = sam_predict_masks(m["dec"], image_embed, prompt_embed, dense_prompt)
    return m.graph.output(masks, "masks"), m.graph.output(iou, "iou")


# ---- SAM3 vision encoder and CLIP text encoder against this layer (the structure of src/visp/arch/sam3.h) ----------------------------------------------
# Node for node, with these departures. Maps are CWHN here, so the reference's WHCN reshape / permute / cont behind the patch conv (sam3.h:320-323) is one
# reshape, and the conv itself (kernel == stride on the f32 image) is the PATCH_EMBED node. The rope positions are i32 CONSTANTS under the reference's names
# (it fills graph inputs on the host, :391-411), and the sine position embedding is an f32 constant computed on the host, CWHN (:524-564 fills a WHCN input).
# The causal mask [T, T, 1, 1] f16 and the token ids [T] (or [T, B]) i32 are graph inputs; the CLIP tokenizer is not part of this layer.

ROPE_TYPE_NORMAL = 0  # GGML_ROPE_TYPE_NORMAL: adjacent pairs


def rope(m, x, pos, n_dims, freq_base, freq_scale):  # ggml_rope_ext in GGML_ROPE_TYPE_NORMAL; pos an i32 constant [T]
    return m.graph.op(OP_ROPE, [x, pos], [n_dims, ROPE_TYPE_NORMAL], [freq_base, freq_scale])


class Sam3VitParams:  # sam3_vit_params, sam3.h:299-307
    def __init__(self, image_size=1008, patch_size=14, window_size=24, n_layers=32, n_heads=16, global_attn_indexes=(7, 15, 23, 31)):
        self.image_size, self.patch_size, self.window_size, self.n_layers, self.n_heads = image_size, patch_size, window_size, n_layers, n_heads
        self.global_attn_indexes = tuple(global_attn_indexes)


def clip_text_embed(m: ModelRef, ids: Tensor) -> Tensor:  # sam3.h:221-231; ids i32 [T] or [T, B], a graph input
    seq_len = ids.ne[0]
    token_embeds = get_rows(m, m.weights("token_embedding.weight"), ids)
    pos_embeds = slice_(m, m.weights("position_embedding.weight"), SLICE_ALL, (0, seq_len))
    return add(m, token_embeds, pos_embeds)


def clip_attention(m: ModelRef, x: Tensor, attention_mask: Tensor, n_heads: int = 16) -> Tensor:  # sam3.h:233-247
    head_dim = x.ne[0] // n_heads
    q, k, v = (reshape(m, linear(m[name], x), head_dim, n_heads, x.ne[1], x.ne[2]) for name in ("q_proj", "k_proj", "v_proj"))
    return attention(m, q, k, v, attention_mask, 1.0 / math.sqrt(float(head_dim)), m["out_proj"])


def clip_mlp(m: ModelRef, x: Tensor) -> Tensor:  # sam3.h:249-254
    return linear(m["fc2"], gelu(m, linear(m["fc1"], x)))


def clip_encoder_layer(m: ModelRef, x: Tensor, attention_mask: Tensor, n_heads: int = 16) -> Tensor:  # sam3.h:256-267
    x = add(m, clip_attention(m["self_attn"], layer_norm(m["layer_norm1"], x), attention_mask, n_heads), x)
    return add(m, clip_mlp(m["mlp"], layer_norm(m["layer_norm2"], x)), x)


def clip_text_encode(m: ModelRef, embeds: Tensor, attention_mask: Tensor, n_heads: int = 16) -> Tensor:  # sam3.h:269-275 (24 layers in SAM3: counted from the weights)
    layers, i = m["layers"], 0
    while layers[i].find("layer_norm1.weight") is not None:
        embeds = clip_encoder_layer(layers[i], embeds, attention_mask, n_heads)
        i += 1
    return embeds


def clip_encode_text(m: ModelRef, ids: Tensor, attention_mask: Tensor, n_heads: int = 16) -> Tensor:  # sam3.h:277-282
    embeds = clip_text_embed(m["embeddings"], ids)
    encoded = clip_text_encode(m["encoder"], embeds, attention_mask, n_heads)
    return layer_norm(m["final_layer_norm"], encoded)


def sam3_encode_text(m: ModelRef, ids: Tensor, attention_mask: Tensor, n_heads: int = 16) -> Tensor:  # sam3.h:284-288; m = "det"
    return linear(m["text_projection"], clip_encode_text(m["te.text_model"], ids, attention_mask, n_heads))


def clip_causal_mask(n_tokens: int, max_tokens: int) -> np.ndarray:
    """The mask clip_tokenizer::tokenize builds (sam3.h:146-192) for a prompt of n_tokens ids (bos and eos included): causal on the prompt's rows, the
    padding rows see the whole prompt. f16 [max_tokens, max_tokens] of 0 / -inf."""
    mask = np.full((max_tokens, max_tokens), -np.inf, np.float16)
    for row in range(max_tokens):
        mask[row, : (row + 1 if row < n_tokens else n_tokens)] = 0
    return mask


def sam3_vision_embed(m: ModelRef, image: Tensor, patch_size: int) -> Tensor:  # sam3.h:313-338; image f32 [3, W, H, N]
    c, w, h, b = image.ne
    wp, hp = w // patch_size, h // patch_size
    embed = patch_embed(m["patch_embeddings"], image, patch_size)
    embed = reshape(m, embed, embed.ne[0], wp * hp, b)
    pos_embed = m.weights("position_embeddings")
    hidden_size = pos_embed.ne[0]
    pretrain_size = int(math.sqrt(float(pos_embed.ne[1])) + 0.5)
    if wp == pretrain_size and hp == pretrain_size:
        pos_embed = reshape(m, pos_embed, hidden_size, wp * hp, 1)
    else:  # tile the position embeddings to the image's grid
        pos_embed = reshape(m, pos_embed, hidden_size, pretrain_size, pretrain_size, 1)
        pos_embed = repeat(m, pos_embed, hidden_size, wp, hp, 1)
        pos_embed = reshape(m, pos_embed, hidden_size, wp * hp, 1)
    return named(m, add(m, embed, pos_embed))


def sam3_mlp(m: ModelRef, x: Tensor) -> Tensor:  # sam3.h:340-345
    return linear(m["fc2"], gelu(m, linear(m["fc1"], x)))


def sam3_window_partition(m: ModelRef, x: Tensor, window: int) -> Tensor:  # sam3.h:347-366
    c, w, h, b = x.ne
    px, py = (window - w % window) % window, (window - h % window) % window
    npw, nph = (w + px) // window, (h + py) // window
    if px > 0 or py > 0:
        x = pad(m, x, 0, px, py, 0)
    x = reshape(m, x, c * window, npw, window, nph * b)
    x = cont(m, permute(m, x, 0, 2, 1, 3))
    return reshape(m, x, c, window * window, npw * nph * b)


def sam3_window_reverse(m: ModelRef, x: Tensor, w: int, h: int, window: int, b: int) -> Tensor:  # sam3.h:368-389 (b: the reference reads ne[3] of a 3-D tensor)
    c = x.ne[0]
    px, py = (window - w % window) % window, (window - h % window) % window
    npw, nph = (w + px) // window, (h + py) // window
    x = reshape(m, x, c * window, window, npw, nph * b)
    x = cont(m, permute(m, x, 0, 2, 1, 3))
    x = reshape(m, x, c, w + px, h + py, b)
    if px > 0 or py > 0:
        x = cont(m, slice_(m, x, SLICE_ALL, (0, w), (0, h)))
    return x


class Rope2dPositions:  # rope_2d_positions, sam3.h:293-297
    def __init__(self, x: Tensor, y: Tensor, scale: float):
        self.x, self.y, self.scale = x, y, scale


def sam3_rope_2d_positions(m: ModelRef, n_pos: int, n_rows: int, scale: float, name: str) -> Rope2dPositions:  # sam3.h:391-411: i32 constants "<name>.x", "<name>.y"
    g, i = m.graph, np.arange(n_pos, dtype=np.int32)
    px = g.get_tensor(f"{name}.x") or g.add_weight(f"{name}.x", i % n_rows, I32)
    py = g.get_tensor(f"{name}.y") or g.add_weight(f"{name}.y", i // n_rows, I32)
    return Rope2dPositions(px, py, scale)


def sam3_apply_rope_2d(m: ModelRef, x: Tensor, pos: Rope2dPositions) -> Tensor:  # sam3.h:413-438: x positions on the first half of a head, y on the second
    freq_base, dim = 10000.0, x.ne[0]
    first = rope(m, slice_(m, x, (0, dim // 2)), pos.x, dim // 2, freq_base, pos.scale)
    second = rope(m, slice_(m, x, (dim // 2, dim)), pos.y, dim // 2, freq_base, pos.scale)
    return concat(m, [first, second], 0)


def sam3_rope_attention(m: ModelRef, x: Tensor, n_heads: int, pos: Rope2dPositions) -> Tensor:  # sam3.h:440-455
    head_dim = x.ne[0] // n_heads
    q, k, v = (reshape(m, linear(m[name], x), head_dim, n_heads, x.ne[1], x.ne[2]) for name in ("q_proj", "k_proj", "v_proj"))
    q, k = sam3_apply_rope_2d(m, q, pos), sam3_apply_rope_2d(m, k, pos)
    return attention(m, q, k, v, None, 1.0 / math.sqrt(float(head_dim)), m["o_proj"])


def sam3_vision_layer(m: ModelRef, x: Tensor, window_size: int, n_heads: int, rope_pos: Rope2dPositions) -> Tensor:  # sam3.h:457-483; x [C, W, H, B]
    residual_attn = x
    x = layer_norm(m["layer_norm1"], x)
    c, w, h, b = x.ne
    x = sam3_window_partition(m, x, window_size) if window_size > 0 else reshape(m, x, c, w * h, b)
    x = sam3_rope_attention(m["attention"], x, n_heads, rope_pos)
    x = sam3_window_reverse(m, x, w, h, window_size, b) if window_size > 0 else reshape(m, x, c, w, h, b)
    x = add(m, x, residual_attn)
    x = add(m, sam3_mlp(m["mlp"], layer_norm(m["layer_norm2"], x)), x)
    return named(m, x)


def sam3_vision_transformer(m: ModelRef, image: Tensor, p: Sam3VitParams) -> Tensor:  # sam3.h:485-515
    x = sam3_vision_embed(m["embeddings"], image, p.patch_size)
    c, w, h, b = x.ne[0], image.ne[1] // p.patch_size, image.ne[2] // p.patch_size, image.ne[3]
    x = reshape(m, x, c, w, h, b)
    pos_window = sam3_rope_2d_positions(m, p.window_size ** 2, p.window_size, 1.0, "_vit_rope_pos_window")
    n_rows_global = p.image_size // p.patch_size
    pos_global = sam3_rope_2d_positions(m, n_rows_global ** 2, n_rows_global, float(p.window_size) / float(n_rows_global), "_vit_rope_pos_global")
    x = layer_norm(m["layer_norm"], x)
    for i in range(p.n_layers):
        is_global = i in p.global_attn_indexes
        x = sam3_vision_layer(m["layers"][i], x, 0 if is_global else p.window_size, p.n_heads, pos_global if is_global else pos_window)
    return reshape(m, x, c, w * h, b)


def sam3_sine_position_values(width: int, height: int, n_pos_feats: int, normalize: bool) -> np.ndarray:
    """sam3.h:537-561 in its f32 arithmetic: numpy [2 n_pos_feats, height, width] (y features first), the reference's WHCN tensor."""
    f32 = np.float32
    dim_t = np.power(f32(10000.0), (f32(2.0) * (np.arange(n_pos_feats) // 2).astype(f32) / f32(n_pos_feats))).astype(f32)
    y, x = np.arange(1, height + 1, dtype=f32), np.arange(1, width + 1, dtype=f32)
    if normalize:
        y, x = y / (f32(height) + f32(1e-6)) * f32(2.0 * math.pi), x / (f32(width) + f32(1e-6)) * f32(2.0 * math.pi)
    even = (np.arange(n_pos_feats) % 2 == 0)[:, None]
    ay, ax = (y[None, :] / dim_t[:, None]).astype(f32), (x[None, :] / dim_t[:, None]).astype(f32)
    fy, fx = np.where(even, np.sin(ay), np.cos(ay)).astype(f32), np.where(even, np.sin(ax), np.cos(ax)).astype(f32)
    out = np.empty((2 * n_pos_feats, height, width), f32)
    out[:n_pos_feats], out[n_pos_feats:] = fy[:, :, None], fx[:, None, :]
    return out


def sam3_sine_position_embedding(m: ModelRef, shape, n_pos_feats: int, normalize: bool) -> Tensor:  # sam3.h:524-564; shape = the map's (C, W, H, N)
    _, width, height, _ = shape
    name = f"_sine_pos_embed_{width}x{height}x{n_pos_feats}{'_norm' if normalize else ''}"
    pe = m.graph.get_tensor(name)
    if pe is None:  # CWHN: [2 F, W, H, 1]
        pe = m.graph.add_weight(name, sam3_sine_position_values(width, height, n_pos_feats, normalize).transpose(1, 2, 0)[None], F32)
    return pe


def sam3_fpn_layer(m: ModelRef, x: Tensor, index: int) -> Tensor:  # sam3.h:566-587
    if index == 0:  # scale factor 4
        x = conv_transpose_2d(m["scale_layers.0"], x, 2)
        x = gelu(m, x)
        x = conv_transpose_2d(m["scale_layers.2"], x, 2)
    elif index == 1:  # scale factor 2
        x = conv_transpose_2d(m["scale_layers.0"], x, 2)
    elif index == 3:  # scale factor 0.5
        x = pool_2d(m, x, POOL_MAX, 2, 2, 2, 2, 0, 0)
    elif index != 2:
        raise ValueError(f"Invalid FPN layer index {index}")
    x = conv_2d(m["proj1"], x, 1, 0)
    return conv_2d(m["proj2"], x, 1, 1)


def sam3_vision_neck(m: ModelRef, x: Tensor):  # sam3.h:589-602 -> (fpn_hidden_states, fpn_position_encoding), four each
    hidden, pos = [], []
    for i in range(4):
        hidden.append(sam3_fpn_layer(m["fpn_layers"][i], x, i))
        pos.append(sam3_sine_position_embedding(m, hidden[i].ne, hidden[i].ne[0] // 2, True))
    return hidden, pos


def sam3_encode_vision(m: ModelRef, image: Tensor, p: Sam3VitParams):  # sam3.h:604-613; m = "det.ve"; image f32 [3, W, H, N]
    c, w, h, b = image.ne
    x = sam3_vision_transformer(m["backbone"], image, p)
    x = reshape(m, x, x.ne[0], w // p.patch_size, h // p.patch_size, b)
    return sam3_vision_neck(m["neck"], x)
