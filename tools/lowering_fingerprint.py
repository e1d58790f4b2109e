"""Fingerprints of what the graph lowering produces, for comparing two builds of the library (a refactor of csrc/lower_*.cpp must not move
any of them). One line per case: the sha256 of `describe()` (launch list + launches / nodes / buffers / arena_bytes / unshared_bytes /
constant_bytes) of a planning-only graph, or the error text where a graph does not lower. No device is needed for these.

With --device the weight arenas of Depth-Anything SMALL and ESRGAN_TINY (fixed seeds) are copied back and hashed -- pack order and pack
contents -- and so are the two models' outputs on fixed inputs; then the small planning cases (RUN) run as graphs on inputs from fixed seeds
and every output's bytes are hashed: a description does not show a launch's arguments, what the launch computes does.

Usage: python tools/lowering_fingerprint.py [--device] [--out FILE] [substring of the case names to run ...]
       VISP_LIBRARY=/path/to/other/libvisioncpp.so selects the build."""
import argparse
import hashlib
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402

load_package()
import numpy as np  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import graph as G  # noqa: E402
from visioncpp_amd import synth  # noqa: E402

import graph_cases as GC  # noqa: E402


def sha(data) -> str:
    return hashlib.sha256(data if isinstance(data, (bytes, bytearray, memoryview)) else str(data).encode()).hexdigest()


def planned(build) -> str:
    try:
        g = build(None)[0]
        g.allocate()
        text = g.describe()
        return f"{sha(text)} {text.strip().splitlines()[-1]}"
    except L.Error as e:
        return f"error: {e}"


def tensors(d):
    """(inputs, outputs) of what a tests/graph_cases.py builder returns"""
    return [d[k] for k in ("x", "other", "image", "src") if k in d], [d[k] for k in ("x0", "y") if k in d] + list(d.get("outs", []))


# the cases small enough to run as well (--device): every name that starts with one of these
RUN = ("yolov9t_96_b2", "migan_32", "tinyvit_mini_b2", "deform_module", "swin_block_mini", "swin_encode_mini", "conv_relu_add", "residual_unit_on_planes",
       "relu_into_output_conv", "conv_narrow_input", "encoder_chain_equal_scales")


def cases(tmp: Path):
    """name, build(device) -> (graph before allocate, its inputs, its outputs)"""
    for cfg in (synth.MINI, synth.TINY, synth.SMALL, synth.BASE, synth.LARGE):
        side = cfg.image_size - cfg.image_size % cfg.patch_size
        path = None
        for w, h in ((side, side), (518, 784)):  # 784 / 14 = 56 patches: the 1/7-level map is 112 px on that side
            for fused in (True, False):
                def build(dev, cfg=cfg, w=w, h=h, fused=fused):
                    nonlocal path
                    path = path or synth.write_gguf(tmp / f"{cfg.name}.gguf", cfg, seed=0)
                    g = G.Graph(dev, G.Weights(path))
                    g.set_fused_models(fused)
                    image = g.input((3, w, h, 2), G.F32, "image")
                    return g, [image], [G.depthany_predict(G.ModelRef(g), image, cfg.n_layers, cfg.n_heads, cfg.patch_size, cfg.feature_layers)]
                yield f"depthany_{cfg.name}_{w}x{h}_{'fused' if fused else 'per_node'}", build
    for cfg in (synth.ESRGAN_TINY, synth.ESRGAN_X4):
        def build(dev, cfg=cfg):
            g = G.Graph(dev, G.Weights(synth.write_esrgan_gguf(tmp / f"esrgan_{cfg.name}.gguf", cfg, 7)))
            image = g.input((3, 40, 56, 3), G.F32, "image")
            return g, [image], [G.esrgan_generate(G.ModelRef(g), image, cfg.scale, cfg.num_blocks)]
        yield f"esrgan_{cfg.name}_40x56", build

    def case(fn, *args):
        def build(dev):
            g = G.Graph(dev)
            return (g, *tensors(fn(g, np.random.default_rng(0), *args)))
        return build
    yield "conv_relu_add_64", case(GC.conv_relu_add, 64)
    yield "conv_relu_add_32", case(GC.conv_relu_add, 32)
    yield "residual_unit_on_planes", case(GC.residual_unit_on_planes)
    yield "relu_into_output_conv_nhwc", case(GC.relu_into_output_conv, False)
    yield "relu_into_output_conv_planar", case(GC.relu_into_output_conv, True)
    yield "conv_leaky_0.2", case(GC.conv_leaky, 0.2)
    yield "conv_leaky_0.1", case(GC.conv_leaky, 0.1)
    yield "encoder_chain_equal_scales", case(GC.encoder_chain, [0.125, 0.125])
    yield "encoder_chain_differing_scales", case(GC.encoder_chain, [0.125, 0.25])
    for cfg, batch in ((synth.TINYVIT_MINI, 2), (synth.TINYVIT_5M, 1)):
        path = None
        for fused in (True, False):
            def build(dev, cfg=cfg, batch=batch, fused=fused):
                nonlocal path
                path = path or synth.write_tinyvit_gguf(tmp / f"tinyvit_{cfg.name}.gguf", cfg, seed=3)
                g = G.Graph(dev, G.Weights(path))
                g.set_fused_models(fused)
                image = g.input((3, cfg.img_size, cfg.img_size, batch), G.F32, "image")
                return g, [image], [g.output(G.tinyvit_encode(G.ModelRef(g, "enc"), image, cfg.layers()), "output")]
            yield f"tinyvit_{cfg.name}_b{batch}_{'fused' if fused else 'per_node'}", build
    ypath = None
    for size, batch in ((96, 2), (640, 1)):
        for fused in (True, False):
            def build(dev, size=size, batch=batch, fused=fused):
                nonlocal ypath
                ypath = ypath or synth.write_yolov9t_gguf(tmp / "yolov9t.gguf", seed=1)
                g = G.Graph(dev, G.Weights(ypath))
                g.set_fused_models(fused)
                image = g.input((3, size, size, batch), G.F32, "image")
                boxes, scores, raw, _ = G.yolov9t_forward(G.ModelRef(g), image)
                return g, [image], [g.output(t, f"out{i}") for i, t in enumerate([boxes, scores, *raw])]
            yield f"yolov9t_{size}_b{batch}_{'fused' if fused else 'per_node'}", build
    for res, kw in ((32, dict(ch_base=256, ch_max=24)), (512, {})):  # widths 8 .. 24 (no multiple of 64), and the full-size generator
        mpath = None
        for fused in (True, False):
            def build(dev, res=res, kw=kw, fused=fused):
                nonlocal mpath
                mpath = mpath or synth.write_migan_gguf(tmp / f"migan_{res}.gguf", res, seed=1, **kw)
                g = G.Graph(dev, G.Weights(mpath))
                g.set_fused_models(fused)
                image = g.input((4, res, res, 2), G.F32, "image")
                return g, [image], [G.migan_generate(G.ModelRef(g), image, res)]
            yield f"migan_{res}_{'fused' if fused else 'per_node'}", build
    # (the per-node module is the one case whose products write ragged rows: gemm_like's unpad_rows)
    spath = None
    for name, fn in (("deform_module", GC.deform_module), ("swin_block_mini", GC.swin_block_mini), ("swin_encode_mini", GC.swin_encode_mini)):
        for fused in (True, False):
            def build(dev, name=name, fn=fn, fused=fused):
                nonlocal spath
                if name != "deform_module":
                    spath = spath or synth.write_swin_gguf(tmp / "swin_mini.gguf", synth.SWIN_MINI, seed=5)
                g = G.Graph(dev, G.Weights(spath) if name != "deform_module" else None)
                g.set_fused_models(fused)
                return (g, *tensors(fn(g)))
            yield f"{name}_{'fused' if fused else 'per_node'}", build
    yield "conv_narrow_input_16", case(GC.conv_narrow_input, 16)
    yield "conv_narrow_input_48", case(GC.conv_narrow_input, 48)


def ran(build, dev, seed) -> str:
    """the graph on the device, on inputs from a fixed seed: the sha256 of every output's bytes"""
    g, ins, outs = build(dev)
    g.allocate()
    rng = np.random.default_rng(seed)
    for t in ins:
        g.set(t, rng.uniform(0.0, 1.0, t.ne[::-1]) if t.dtype == G.F32 else 0.5 * rng.standard_normal(t.ne[::-1]))
    g.compute()
    return " ".join(sha(np.ascontiguousarray(g.get(t)).tobytes()) for t in outs)


def device_cases(tmp: Path, only):
    from visioncpp_amd import vision

    dev = vision.Device.init(vision.Backend.gpu)

    def arena(model):
        ptr, n = model.weights_arena()
        host = np.empty(n, np.uint8)
        L.vx_check(L.get_lib().vx_memcpy_d2h(host.ctypes.data, ptr, n, None))
        L.vx_check(L.get_lib().vx_stream_sync(None))
        return f"{sha(host.tobytes())} bytes={n}"

    model = vision.Model.load(synth.write_gguf(tmp / "dev_small.gguf", synth.SMALL, seed=0), dev)
    yield "device_depthany_small_arena", arena(model)
    out, raw = model.compute_batch(synth.images(2, 518, 518, seed=12), return_raw=True)
    yield "device_depthany_small_output_518x518", sha(np.ascontiguousarray(out).tobytes()) + " raw " + sha(np.ascontiguousarray(raw).tobytes())
    out = model.compute_batch(synth.images(2, 784, 518, seed=13))
    yield "device_depthany_small_output_784x518", sha(np.ascontiguousarray(out).tobytes())
    emodel = vision.Model.load(synth.write_esrgan_gguf(tmp / "dev_esrgan_tiny.gguf", synth.ESRGAN_TINY, seed=7), dev)
    yield "device_esrgan_tiny_arena", arena(emodel)
    yield "device_esrgan_tiny_output_72x56", sha(np.ascontiguousarray(emodel.upscale_batch(synth.images(1, 72, 56, seed=5))).tobytes())
    for i, (name, build) in enumerate(cases(tmp)):
        if name.startswith(RUN) and (not only or any(s in name for s in only)):
            yield f"device_graph_{name}", ran(build, dev, 100 + i)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", action="store_true", help="also hash the weight arenas and outputs of two models on the GPU")
    ap.add_argument("--out", help="write the lines to this file as well")
    ap.add_argument("only", nargs="*", help="run the cases whose name contains one of these")
    args = ap.parse_args()
    lines = []

    def put(name, value):
        lines.append(f"{name}: {value}")
        print(lines[-1], flush=True)

    with tempfile.TemporaryDirectory() as td:
        for name, build in cases(Path(td)):
            if not args.only or any(s in name for s in args.only):
                put(name, planned(build))
        if args.device:
            for name, value in device_cases(Path(td), args.only):
                put(name, value)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
