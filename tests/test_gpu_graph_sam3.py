"""-m gpu: the rotation and gather kernels of csrc/kernels_rope.hip (vx_rope_f16, vx_rope2d_f16, vx_get_rows_f16, vx_rope_supported, vx_rope2d_supported), the ROPE and get_rows
nodes, the rope_2d group, and the SAM3 vision encoder and CLIP text encoder built through vision.cpp_amd/graph.py -- against float64 numpy
(tests/sam3_ref.py, pinned to `transformers` by tests/test_sam3_ref_cpu.py).

Kernel allowance, per element, from the arithmetic: |got - ref| <= 2^-11 |ref| + 2^-21 (|x0| + |x1|) |q_scale| + 2^-25 -- one f16 rounding; at most five f32
roundings (the two table entries, a product, an fma, the scale) of terms no larger than (|x0| + |x1|) |q_scale|, covered by eight; the f16 subnormal step.
ref is float64 on the f16 inputs with float64 cos and sin. Every element of the output buffer is compared, and a guard region behind it must stay as it was
filled. The ROPE node and the rope_2d group are held to the same allowance in both lowering modes: the slice and concat copies of the per-node path move bits
and round nothing, so the second ulp a rounding per stage would need is not granted.

The encoders: sam3_ref runs once exact and once with f16() applied to every node's output (where the per-node plan holds an f16 buffer); the distance of the
two -- largest absolute error over largest reference value -- is the pipeline's f16 floor, computed with no code under test. The device may be at most
4 x that floor, fused and per node, and the two modes agree within twice that bound. Floors, errors and ratios are printed at module
teardown (and written to the file VISP_SAM3_RATIOS names); profiles/sam3_graph_ratios.txt holds the MI355X's."""
import os

import numpy as np
import pytest

import sam3_ref as R
from visioncpp_amd import _lib as L
from visioncpp_amd import graph as G
from visioncpp_amd import synth, vision

pytestmark = pytest.mark.gpu

from gpu_util import api, dev, empty, release, sync  # noqa: E402

MODES = pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_node"])
VIT, CLIP = synth.SAM3_VIT_MINI, synth.CLIP_TEXT_MINI
GUARD = 256          # f16 elements behind every output buffer
GUARD_BITS = 0x7B7B  # what they are filled with
_ratios: list[str] = []


@pytest.fixture(scope="module")
def device():
    assert api().vx_device_count() > 0, "no HIP device visible: the product path has no CPU fallback"
    return vision.Device.init(vision.Backend.gpu)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    release()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    text = "\n".join(_ratios) + "\n"
    print("\n" + text)
    if os.environ.get("VISP_SAM3_RATIOS"):
        with open(os.environ["VISP_SAM3_RATIOS"], "w") as f:
            f.write(text)


def _i64(v):
    import ctypes
    return (ctypes.c_int64 * len(v))(*[int(x) for x in v])


# ---- the kernels against float64 ----------------------------------------------------------------------------------------------------------------------------

_case_cache = {}


def _case(case):
    """q, k, their float64 rotations (unscaled) and the two f32 tables: computed once per case, shared, read-only."""
    name, hd, heads, T, B, (px, py), scale = case
    if name not in _case_cache:
        q, k = R.rope_case_data(case)
        rq, rk = R.rope_2d(q.astype(np.float64), px, py, R.ROPE_BASE, scale), R.rope_2d(k.astype(np.float64), px, py, R.ROPE_BASE, scale)
        tx, ty = R.rope_table(px, hd // 2, R.ROPE_BASE, scale), R.rope_table(py, hd // 2, R.ROPE_BASE, scale)
        for a in (q, k, rq, rk, tx, ty):
            a.setflags(write=False)
        _case_cache[name] = (q, k, rq, rk, tx, ty)
    return _case_cache[name]


def _guarded(a16: np.ndarray):
    """A device buffer holding a16 followed by the guard pattern."""
    flat = np.concatenate([a16.ravel().view(np.uint16), np.full(GUARD, GUARD_BITS, np.uint16)])
    return dev(flat)


def _read(buf, shape):
    n = int(np.prod(shape))
    flat = buf.to_numpy(np.uint16, (n + GUARD,))
    assert (flat[n:] == GUARD_BITS).all(), "the guard region behind the output was written"
    return flat[:n].view(np.float16).reshape(shape)


def _inside(got, ref, x16, q_scale, label):
    excess = np.abs(got.astype(np.float64) - ref) - R.rope_allowance(ref, x16, q_scale)
    worst = float((np.abs(got.astype(np.float64) - ref) / R.rope_allowance(ref, x16, q_scale)).max())
    print(f"{label}: largest error / allowance {worst:.3f}")
    assert excess.max() <= 0, (label, float(excess.max()))
    return worst


@pytest.mark.parametrize("q_scale", [1.0, R.VX_ATTN_Q_SCALE], ids=["scale1", "attn_scale"])
@pytest.mark.parametrize("case", R.ROPE_CASES, ids=[c[0] for c in R.ROPE_CASES])
def test_rope2d_kernel_against_float64(case, q_scale):
    """vx_rope2d_f16 on q and k in one launch: out of place on token-major rows, and in place on head-major buffers. q_scale goes into q only."""
    name, hd, heads, T, B, _, _ = case
    q, k, rq, rk, tx, ty = _case(case)
    dtx, dty = dev(tx), dev(ty)
    tok = _i64([hd, hd * heads, hd * heads * T])        # (head, token, batch) of [B][T][heads][hd]
    assert api().vx_rope_supported(hd // 2, heads, T, B, tok, tok) == 1
    qo, ko = _guarded(np.zeros_like(q)), _guarded(np.zeros_like(k))
    L.vx_check(api().vx_rope2d_f16(dev(q).ptr, qo.ptr, dev(k).ptr, ko.ptr, dtx.ptr, dty.ptr, hd, heads, T, B, tok, tok, q_scale, None))
    sync()
    worst = _inside(_read(qo, q.shape), rq * q_scale, q, q_scale, f"{name} token-major q")
    worst = max(worst, _inside(_read(ko, k.shape), rk, k, 1.0, f"{name} token-major k"))
    # head-major [B][heads][T][hd], in place: what the fused q|k|v product leaves behind
    head = _i64([hd * T, hd, hd * T * heads])
    qh, kh = np.ascontiguousarray(q.transpose(0, 2, 1, 3)), np.ascontiguousarray(k.transpose(0, 2, 1, 3))
    qb, kb = _guarded(qh), _guarded(kh)
    L.vx_check(api().vx_rope2d_f16(qb.ptr, qb.ptr, kb.ptr, kb.ptr, dtx.ptr, dty.ptr, hd, heads, T, B, head, head, q_scale, None))
    sync()
    worst = max(worst, _inside(_read(qb, qh.shape).transpose(0, 2, 1, 3), rq * q_scale, q, q_scale, f"{name} head-major in place q"))
    worst = max(worst, _inside(_read(kb, kh.shape).transpose(0, 2, 1, 3), rk, k, 1.0, f"{name} head-major in place k"))
    _ratios.append(f"vx_rope2d_f16 {name} hd={hd} heads={heads} T={T} B={B} q_scale={q_scale:.6g}: largest error / allowance {worst:.3f}")


@pytest.mark.parametrize("q_scale", [1.0, R.VX_ATTN_Q_SCALE], ids=["scale1", "attn_scale"])
@pytest.mark.parametrize("case", R.ROPE_CASES, ids=[c[0] for c in R.ROPE_CASES])
def test_rope_kernel_n32_against_float64(case, q_scale):
    """vx_rope_f16 alone, n = 32: each half of the heads, read where it lies in the 64-wide rows (strides in != strides out) into rows of 32, and a
    contiguous copy of the half rotated in place on head-major rows."""
    name, hd, heads, T, B, _, _ = case
    q, _, rq, _, tx, ty = _case(case)
    n = hd // 2
    dq = dev(q)
    worst = 0.0
    for h, tab in enumerate((tx, ty)):
        ref = rq[..., h * n:(h + 1) * n] * q_scale
        x = np.ascontiguousarray(q[..., h * n:(h + 1) * n])
        dt = dev(tab)
        out = _guarded(np.zeros_like(x))
        L.vx_check(api().vx_rope_f16(dq.ptr + 2 * h * n, out.ptr, dt.ptr, n, heads, T, B, _i64([hd, hd * heads, hd * heads * T]), _i64([n, n * heads, n * heads * T]), q_scale, None))
        sync()
        worst = max(worst, _inside(_read(out, x.shape), ref, x, q_scale, f"{name} half {h} out of place"))
        xh = np.ascontiguousarray(x.transpose(0, 2, 1, 3))
        buf = _guarded(xh)
        head = _i64([n * T, n, n * T * heads])
        L.vx_check(api().vx_rope_f16(buf.ptr, buf.ptr, dt.ptr, n, heads, T, B, head, head, q_scale, None))
        sync()
        worst = max(worst, _inside(_read(buf, xh.shape).transpose(0, 2, 1, 3), ref, x, q_scale, f"{name} half {h} in place"))
    _ratios.append(f"vx_rope_f16 {name} n={n} heads={heads} T={T} B={B} q_scale={q_scale:.6g}: largest error / allowance {worst:.3f}")


def test_rope_launcher_refusals():
    """No launch happens: the output keeps its fill."""
    x = np.zeros((1, 4, 2, 32), np.float16)
    dx, out, tab = dev(x), _guarded(np.full(x.shape, 3.0, np.float16)), dev(np.zeros((4, 32), np.float32))
    s = _i64([32, 64, 256])
    fn, fn2 = api().vx_rope_f16, api().vx_rope2d_f16
    for call, msg in [
        (lambda: fn(dx.ptr + 2, out.ptr, tab.ptr, 32, 2, 4, 1, s, s, 1.0, None), b"16-byte aligned"),
        (lambda: fn(dx.ptr, out.ptr + 8, tab.ptr, 32, 2, 4, 1, s, s, 1.0, None), b"16-byte aligned"),
        (lambda: fn(dx.ptr, out.ptr, tab.ptr + 4, 32, 2, 4, 1, s, s, 1.0, None), b"16-byte aligned"),
        (lambda: fn(dx.ptr, out.ptr, tab.ptr, 12, 2, 4, 1, s, s, 1.0, None), b"n = 12"),
        (lambda: fn(dx.ptr, out.ptr, tab.ptr, 32, 2, 0, 1, s, s, 1.0, None), b"empty problem"),
        (lambda: fn(dx.ptr, out.ptr, tab.ptr, 32, 0, 4, 1, s, s, 1.0, None), b"empty problem"),
        (lambda: fn(None, out.ptr, tab.ptr, 32, 2, 4, 1, s, s, 1.0, None), b"null operand"),
        (lambda: fn(dx.ptr, out.ptr, tab.ptr, 32, 2, 4, 1, _i64([32, 60, 256]), s, 1.0, None), b"multiples of 8"),
        (lambda: fn(dx.ptr, out.ptr, tab.ptr, 32, 2, 4, 1 << 20, _i64([32, 64, 1 << 20]), s, 1.0, None), b"32-bit indexing"),
        (lambda: fn(out.ptr, out.ptr, tab.ptr, 32, 2, 4, 1, s, _i64([32, 128, 512]), 1.0, None), b"in place needs equal strides"),
        (lambda: fn(dx.ptr, dx.ptr + 64, tab.ptr, 32, 2, 4, 1, s, s, 1.0, None), b"output 0 overlaps input 0"),
        (lambda: fn2(dx.ptr, out.ptr, out.ptr, dx.ptr, tab.ptr, tab.ptr, 32, 2, 4, 1, s, s, 1.0, None), b"overlaps input"),
        (lambda: fn2(dx.ptr, out.ptr, dx.ptr, out.ptr + 64, tab.ptr, tab.ptr, 32, 2, 4, 1, s, s, 1.0, None), b"the two outputs overlap"),
        (lambda: fn2(dx.ptr, out.ptr, None, None, tab.ptr, tab.ptr, 40, 2, 4, 1, s, s, 1.0, None), b"head_dim 40"),
        (lambda: fn2(dx.ptr, out.ptr, dx.ptr, None, tab.ptr, tab.ptr, 32, 2, 4, 1, s, s, 1.0, None), b"null operand"),
        (lambda: api().vx_get_rows_f16(dx.ptr, tab.ptr, out.ptr, 4, 12, 4, None), b"C = 12"),
        (lambda: api().vx_get_rows_f16(dx.ptr, tab.ptr, out.ptr, 4, 32, 0, None), b"empty problem"),
        (lambda: api().vx_get_rows_f16(dx.ptr + 2, tab.ptr, out.ptr, 4, 32, 4, None), b"16-byte aligned"),
    ]:
        assert call() == 0 and msg in api().vx_last_error(), (msg, api().vx_last_error())
    assert api().vx_rope2d_supported(32, 2, 4, 1, s, s) == 1 and api().vx_rope2d_supported(40, 2, 4, 1, s, s) == 0 and api().vx_rope2d_supported(32, 2, 4, 0, s, s) == 0
    assert api().vx_rope_supported(12, 2, 4, 1, s, s) == 0 and api().vx_rope_supported(32, 2, 0, 1, s, s) == 0 and api().vx_rope_supported(32, 2, 4, 1, s, s) == 1
    sync()
    assert (_read(out, x.shape) == 3.0).all()


IDS = [np.array([0, 99, 5, 5, 17, 0, 99, 42], np.int32), np.array([[0, 1, 2, 3, 99, 99, 99, 99], [98, 0, 98, 0, 50, 50, 7, 99], [3, 3, 3, 3, 3, 3, 3, 3]], np.int32)]


@pytest.mark.parametrize("ids", IDS, ids=["T", "T_B"])
def test_get_rows_kernel_and_node_are_bit_exact(device, ids):
    """Ids include 0, rows - 1 and repeats; against numpy indexing of the f16-rounded table, bit for bit."""
    table = np.random.default_rng(11).standard_normal((100, 128)).astype(np.float32)
    t16 = table.astype(np.float16)
    want = t16[ids]
    out = _guarded(np.zeros(want.shape, np.float16))
    L.vx_check(api().vx_get_rows_f16(dev(t16).ptr, dev(ids).ptr, out.ptr, 100, 128, ids.size, None))
    sync()
    assert np.array_equal(_read(out, want.shape).view(np.uint16), want.view(np.uint16))
    for fused in (True, False):
        g = G.Graph(device)
        g.set_fused_models(fused)
        y = g.output(G.get_rows(G.ModelRef(g), g.add_weight("table", table), idx := g.input(ids.shape[::-1], G.I32, "ids")), "rows")
        g.allocate()
        g.set(idx, ids)
        g.compute()
        got = g.get(y).reshape(want.shape)
        assert np.array_equal(got.astype(np.float16).view(np.uint16), want.view(np.uint16))


# ---- the ROPE node and the rope_2d group ----------------------------------------------------------------------------------------------------------------------

@MODES
@pytest.mark.parametrize("case", [R.ROPE_CASES[i] for i in (1, 2, 3, 5)], ids=[R.ROPE_CASES[i][0] for i in (1, 2, 3, 5)])
def test_rope_2d_group(device, case, fused):
    name, hd, heads, T, B, (px, py), scale = case
    q, _, rq, _, _, _ = _case(case)
    g = G.Graph(device)
    g.set_fused_models(fused)
    m = G.ModelRef(g)
    pos = G.Rope2dPositions(g.add_weight("p.x", px.astype(np.int32), G.I32), g.add_weight("p.y", py.astype(np.int32), G.I32), scale)
    x = g.input((hd, heads, T, B), G.F16, "q")
    y = g.output(G.sam3_apply_rope_2d(m, x, pos), "out")
    g.allocate()
    kinds = [l.split(" ")[0] for l in g.describe().strip().splitlines()[:-1]]
    assert kinds == (["rope_2d"] if fused else ["slice", "rope", "slice", "rope", "concat", "concat"])
    g.set(x, q)
    g.compute()
    worst = _inside(g.get(y).reshape(q.shape).astype(np.float16), rq, q, 1.0, f"rope_2d group {name} {'fused' if fused else 'per node'}")
    _ratios.append(f"rope_2d group {name} {'fused' if fused else 'per node'}: largest error / allowance {worst:.3f}")


@MODES
def test_rope_node(device, fused):
    """One ROPE node, n = 32, odd T, arbitrary positions at scale 1 / 3."""
    rng = np.random.default_rng(21)
    x16 = rng.standard_normal((2, 25, 3, 32)).astype(np.float16)
    pos = rng.integers(0, 72, 25).astype(np.int32)
    g = G.Graph(device)
    g.set_fused_models(fused)
    x = g.input((32, 3, 25, 2), G.F16, "x")
    y = g.output(G.rope(G.ModelRef(g), x, g.add_weight("pos", pos, G.I32), 32, 10000.0, 1.0 / 3.0), "y")
    g.allocate()
    assert g.describe().strip().splitlines()[:-1] == ["rope n=32 heads=3 T=25 B=2"]
    g.set(x, x16)
    g.compute()
    _inside(g.get(y).reshape(x16.shape).astype(np.float16), R.rope(x16.astype(np.float64), pos, 32, 10000.0, 1.0 / 3.0), x16, 1.0, "rope node")


# ---- the encoders against sam3_ref ---------------------------------------------------------------------------------------------------------------------------

def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / np.abs(want).max())


_weights_cache = {}


def _tensors(kind):
    if kind not in _weights_cache:
        sd = synth.sam3_vision_state_dict(VIT, 1) if kind == "vit" else synth.clip_text_state_dict(CLIP, 2)
        _weights_cache[kind] = synth.sam3_graph_tensors(sd)
    return _weights_cache[kind]


def _graph(device, kind, fused):
    g = G.Graph(device)
    g.set_fused_models(fused)
    for name, t in _tensors(kind).items():
        g.add_weight(name, t)
    return g, G.ModelRef(g)


def _judge(label, results, exact, floored):
    """results: {mode: array}. The floor from the reference alone; every mode within 4 x floor; the modes within 8 x floor of each other."""
    floor = _rel(floored, exact)
    assert floor > 0
    for mode, got in results.items():
        err = _rel(got, exact)
        _ratios.append(f"{label} {mode}: floor {floor:.3e} error {err:.3e} ratio {err / floor:.2f}")
        print(_ratios[-1])
    for mode, got in results.items():
        assert _rel(got, exact) <= 4 * floor, (label, mode, _rel(got, exact), floor)
    if len(results) == 2:
        a, b = results.values()
        assert _rel(a, np.asarray(b, np.float64)) * np.abs(b).max() / np.abs(exact).max() <= 8 * floor, label


LAYER_CASES = [("window", 4, 8, 0), ("global", 0, 8, 1), ("padded", 4, 6, 0)]


@pytest.mark.parametrize("name, window, grid, layer", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_vision_layer(device, name, window, grid, layer):
    x16 = np.random.default_rng(31).standard_normal((2, grid, grid, VIT.hidden)).astype(np.float16)
    n = window if window else grid
    px, py = R.rope_2d_positions(n * n, n)
    scale = 1.0 if window else VIT.window / grid
    p = f"det.ve.backbone.layers.{layer}"
    exact = R.vision_layer(_tensors("vit"), p, x16.astype(np.float64), window, VIT.heads, (px, py, scale))
    floored = R.vision_layer(_tensors("vit"), p, x16.astype(np.float64), window, VIT.heads, (px, py, scale), R.f16)
    results = {}
    for fused in (True, False):
        g, m = _graph(device, "vit", fused)
        x = g.input((VIT.hidden, grid, grid, 2), G.F16, "x")
        pos = G.sam3_rope_2d_positions(m, n * n, n, scale, "pos")
        y = g.output(G.sam3_vision_layer(m[p], x, window, VIT.heads, pos), "y")
        g.allocate()
        lines = g.describe()
        assert ("rope_2d[q k heads-major, in place]" in lines) == fused and (lines.count("\nrope n=32") == 4) == (not fused)
        g.set(x, x16)
        g.compute()
        results["fused" if fused else "per node"] = g.get(y).reshape(exact.shape)
    _judge(f"vision layer {name}", results, exact, floored)


def _encode_vision(device, fused, images):
    g, m = _graph(device, "vit", fused)
    image = g.input((3, VIT.image_size, VIT.image_size, images.shape[0]), G.F32, "image")
    params = G.Sam3VitParams(VIT.image_size, VIT.patch, VIT.window, VIT.n_layers, VIT.heads, VIT.global_layers)
    hidden, pos = G.sam3_encode_vision(m["det.ve"], image, params)
    outs = [g.output(h, f"fpn_{i}") for i, h in enumerate(hidden)]
    g.allocate()
    g.set(image, images)
    g.compute()
    return [g.get(o) for o in outs], [g.read_constant(p)[0] for p in pos]


def test_vision_encoder_and_neck(device):
    images = np.random.default_rng(41).standard_normal((2, VIT.image_size, VIT.image_size, 3)).astype(np.float32)
    w = _tensors("vit")
    exact_h, exact_p = R.encode_vision(w, "det.ve", images, VIT)
    floor_h, _ = R.encode_vision(w, "det.ve", images, VIT, R.f16)
    fused, pos = _encode_vision(device, True, images)
    per_node, _ = _encode_vision(device, False, images)
    for i in range(4):
        _judge(f"vision encoder fpn {i}", {"fused": fused[i], "per node": per_node[i]}, exact_h[i], floor_h[i])
        assert _rel(pos[i], exact_p[i]) < 1e-5, i  # the sine position encoding: an f32 constant computed on the host
    # two images as a batch give each image the bits it gets alone
    for b in range(2):
        alone, _ = _encode_vision(device, True, images[b:b + 1])
        for i in range(4):
            assert np.array_equal(alone[i][0].view(np.uint32), fused[i][b].view(np.uint32)), (b, i)


def test_text_encoder(device):
    rng = np.random.default_rng(51)
    ids = rng.integers(1, CLIP.vocab - 1, (2, CLIP.positions)).astype(np.int32)
    ids[:, 0], ids[:, 4:] = 0, CLIP.vocab - 1  # bos, ..., eos and padding
    mask = G.clip_causal_mask(5, CLIP.positions)
    w = _tensors("clip")
    exact = R.encode_text(w, "det", ids, mask.astype(np.float64), CLIP.heads)
    floored = R.encode_text(w, "det", ids, mask.astype(np.float64), CLIP.heads, R.f16)
    results = {}
    for fused in (True, False):
        g, m = _graph(device, "clip", fused)
        t_ids, t_mask = g.input((CLIP.positions, 2), G.I32, "ids"), g.input((CLIP.positions, CLIP.positions, 1, 1), G.F16, "mask")
        y = g.output(G.sam3_encode_text(m["det"], t_ids, t_mask, CLIP.heads), "text")
        g.allocate()
        g.set(t_ids, ids)
        g.set(t_mask, mask)
        g.compute()
        results["fused" if fused else "per node"] = g.get(y).reshape(exact.shape)
    _judge("text encoder", results, exact, floored)
    # two prompts as a batch give each the bits it gets alone
    g, m = _graph(device, "clip", True)
    t_ids, t_mask = g.input((CLIP.positions, 1), G.I32, "ids"), g.input((CLIP.positions, CLIP.positions, 1, 1), G.F16, "mask")
    y = g.output(G.sam3_encode_text(m["det"], t_ids, t_mask, CLIP.heads), "text")
    g.allocate()
    g.set(t_mask, mask)
    for b in range(2):
        g.set(t_ids, ids[b:b + 1])
        g.compute()
        assert np.array_equal(g.get(y).reshape(exact.shape[1:]).view(np.uint32), results["fused"][b].view(np.uint32)), b
