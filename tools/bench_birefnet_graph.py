#!/usr/bin/env python3
"""Same-device timing of BiRefNet written against the graph layer (vision.cpp_amd/graph.py: birefnet_predict) and of the kernels it brought
(csrc/kernels_imgops.hip), next to the hand schedule's step (csrc/birefnet.cpp) from the same run.

Kernels, at BiRefNet-lite's shapes (1024 x 1024 image, batch 8): the f32 image resize 1024^2 -> 512^2; image_to_patches at the four decoder levels in its naive form
(form 1: a thread gathers 8 channels) and in the form that walks image rows through LDS (form 2); the pixel gate against the per-node chain it replaces (1x1 conv to
one channel, sigmoid, the broadcast copy, the product); the resize and the LayerNorm that write a slice of a concat against the plain launch plus the copy of its result.
Device events
around `reps` launches after three warm-up launches, the variants of a case alternating over `rounds` rounds; median microseconds and the run-to-run spread
(max - min over the rounds). Next to each: the bytes the launch must move (every input once, every output once) and the time those take at 6.3 TB/s. The
operands of one case are tens of megabytes and stay in the 256 MB Infinity Cache between launches: a figure below the HBM byte bound says that, not more.

Network, BiRefNet-lite's shape (1024 x 1024, batch 8 by default: the per-GPU share of BASELINE.json configs[3]) on synth.SWIN_T's depths at embed_dim 64 (stages of
64 / 128 / 256 / 512 channels, heads 2 / 4 / 8 / 16), synthetic weights. Not SWIN_T's own 96: its last patch merging normalises rows of 1536 channels, and the graph
layer's layer_norm takes 1024 at most (a refusal tests/test_depthany_variants_cpu.py pins), so swin_encode does not plan at that width. The graph fused and per node,
each replayed as one hipGraph on the f32 image on the device: a host clock around `steps` computes that end in a device synchronise, after three warm-up computes. The hand schedule: visp_birefnet_compute_batch_device on u8 images (its normalisation included), the same clock. Not the same work at the front
end, so the tool forms no ratio of them. If the graph's arena does not fit the device's free memory the batch is halved until it does, and the record says so.

Prints a text record, writes it to --out, and prints one JSON line last. A measurement, not a gate. On a shared machine run it under a time limit of its own:

    timeout -k 10 900 python tools/bench_birefnet_graph.py [--batch 8] [--size 1024] [--steps 10] [--reps 20] [--rounds 5] [--out profiles/birefnet_graph_bench.txt]"""
import argparse
import ctypes as C
import dataclasses
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from tests import gpu_util as G  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402
from visioncpp_amd import graph as GR  # noqa: E402
from visioncpp_amd import synth, vision  # noqa: E402

HBM = 6.3e12
RECORD = []


def say(text=""):
    RECORD.append(text)
    print(text, flush=True)


def timed(fn, reps):
    api = G.api()
    e0, e1 = C.c_void_p(), C.c_void_p()
    api.vx_event_create(C.byref(e0)); api.vx_event_create(C.byref(e1))
    for _ in range(3):
        fn()
    api.vx_event_record(e0, None)
    for _ in range(reps):
        fn()
    api.vx_event_record(e1, None)
    G.sync()
    ms = C.c_float()
    api.vx_event_elapsed_ms(e0, e1, C.byref(ms))
    api.vx_event_destroy(e0); api.vx_event_destroy(e1)
    return ms.value / reps * 1e3  # us per repetition


def compare(case, variants, nbytes, reps, rounds, same=None):
    """variants: {name: launch function}; alternating over the rounds"""
    t = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            t[k].append(timed(fn, reps))
    row = {"case": case}
    text = f"  {case:44s}"
    for k in variants:
        row[f"{k}_us"], row[f"{k}_spread_us"] = round(float(np.median(t[k])), 1), round(max(t[k]) - min(t[k]), 1)
        row[f"{k}_bytes"], row[f"{k}_byte_bound_us"] = nbytes[k], round(nbytes[k] / HBM * 1e6, 1)
        text += f" {k} {row[f'{k}_us']:8.1f} us (spread {row[f'{k}_spread_us']:5.1f}, byte bound {row[f'{k}_byte_bound_us']:6.1f})"
    if same is not None:
        row["same_bits"] = bool(same)
        text += f"   same bits: {bool(same)}"
    say(text)
    return row


def kernel_cases(B, S, reps, rounds):
    api = G.api()
    rng = np.random.default_rng(0)
    rows = []
    image = G.dev(rng.standard_normal((B, S, S, 3), dtype=np.float32))
    half = G.empty(B * (S // 2) * (S // 2) * 3 * 4)
    rows.append(compare(f"image resize {S}^2 -> {S // 2}^2 x 3", {"resize": lambda: L.vx_check(api.vx_image_bilinear_ac_f32(image.ptr, half.ptr, B, S, S, 3, S // 2, S // 2, None))},
                        {"resize": B * (S * S + S * S // 4) * 12}, reps, rounds))
    n_out = B * S * S * 3  # every level's patch map has as many elements as the image
    out1, out2 = G.empty(n_out * 2, zero=False), G.empty(n_out * 2, zero=False)
    for level in (4, 8, 16, 32):  # the grid: maps of S / 4 .. S / 32
        w = S // level
        naive = lambda w=w: L.vx_check(api.vx_image_patches_f16(image.ptr, out1.ptr, B, S, S, 3, w, w, 1, None))  # noqa: E731
        rowsf = lambda w=w: L.vx_check(api.vx_image_patches_f16(image.ptr, out2.ptr, B, S, S, 3, w, w, 2, None))  # noqa: E731
        naive(); rowsf(); G.sync()
        same = np.array_equal(out1.to_numpy(np.float16, (n_out,)), out2.to_numpy(np.float16, (n_out,)))
        nb = n_out * 4 + n_out * 2
        rows.append(compare(f"image patches {S}^2 -> {w}^2, grid {level} ({level * level * 3} ch, tile {api.vx_image_patches_tile(level * level * 3)})", {"naive": naive, "rows": rowsf},
                            {"naive": nb, "rows": nb}, reps, rounds, same))
    # the gate at a decoder level of BiRefNet-lite: the 1/8 map
    Cc, Cg, side = 192, 16, S // 8
    M = B * side * side
    p, a = G.dev(rng.standard_normal((M, Cc), dtype=np.float32).astype(np.float16)), G.dev(rng.standard_normal((M, Cg), dtype=np.float32).astype(np.float16))
    wv = G.dev(rng.standard_normal(Cg, dtype=np.float32))
    y_f, y_c, logit, gate, wide = G.empty(M * Cc * 2), G.empty(M * Cc * 2), G.empty(M * 4), G.empty(M * 2), G.empty(M * Cc * 2)
    ne, ss, ds = (C.c_int64 * 4)(Cc, M, 1, 1), (C.c_int64 * 4)(0, 1, 0, 0), (C.c_int64 * 4)(1, Cc, 0, 0)

    def fused():
        L.vx_check(api.vx_pixel_gate_f16(p.ptr, Cc, a.ptr, Cg, wv.ptr, C.c_float(0.1), y_f.ptr, Cc, M, Cc, Cg, None))

    def chain():
        L.vx_check(api.vx_conv1x1_to1_f32(a.ptr, wv.ptr, C.c_float(0.1), 0, C.c_float(1.0), logit.ptr, M, Cg, None))
        L.vx_check(api.vx_sigmoid_f16(logit.ptr, 1, gate.ptr, M, None))
        L.vx_check(api.vx_copy_strided_f16(gate.ptr, wide.ptr, ne, ss, ds, C.c_float(1.0), None))
        L.vx_check(api.vx_binary_rows(1, p.ptr, 0, wide.ptr, 0, M * Cc, y_c.ptr, 0, M * Cc, None))

    fused(); chain(); G.sync()
    d = np.abs(y_f.to_numpy(np.float16, (M, Cc)).astype(np.float32) - y_c.to_numpy(np.float16, (M, Cc)).astype(np.float32)).max()
    rows.append(compare(f"pixel gate {side}^2 x {Cc}, Cg {Cg} (max |fused - chain| {d:.2g})", {"fused": fused, "chain": chain},
                        {"fused": M * (2 * Cc + Cg) * 2, "chain": M * (Cg * 2 + 4 + 4 + 2 + 2 + Cc * 2 + 3 * Cc * 2)}, reps, rounds))
    # a resize into its slice of a concat: the half-size pass's 1/8 map (C 192) into channels [192, 384) of the 1/4 feature, against the resize and the copy of its result
    Cc, hs, hd = 192, S // 16, S // 8
    src = G.dev(rng.standard_normal((B, hs, hs, Cc), dtype=np.float32).astype(np.float16))
    cat1, cat2, tmp = G.empty(B * hd * hd * 2 * Cc * 2), G.empty(B * hd * hd * 2 * Cc * 2), G.empty(B * hd * hd * Cc * 2)
    Mo = B * hd * hd
    ne, ss, ds = (C.c_int64 * 4)(Cc, Mo, 1, 1), (C.c_int64 * 4)(1, Cc, 0, 0), (C.c_int64 * 4)(1, 2 * Cc, 0, 0)

    def in_place():
        L.vx_check(api.vx_bilinear_ac_pix_f16(src.ptr, Cc, cat1.ptr + Cc * 2, 2 * Cc, B, hs, hs, Cc, hd, hd, None))

    def resize_copy():
        L.vx_check(api.vx_bilinear_ac_f16(src.ptr, tmp.ptr, B, hs, hs, Cc, hd, hd, None))
        L.vx_check(api.vx_copy_strided_f16(tmp.ptr, cat2.ptr + Cc * 2, ne, ss, ds, C.c_float(1.0), None))

    in_place(); resize_copy(); G.sync()
    same = np.array_equal(cat1.to_numpy(np.float16, (Mo, 2 * Cc)), cat2.to_numpy(np.float16, (Mo, 2 * Cc)))
    n_in, n_o = B * hs * hs * Cc, Mo * Cc
    rows.append(compare(f"resize {hs}^2 -> {hd}^2 x {Cc} into a concat", {"in_place": in_place, "resize_copy": resize_copy}, {"in_place": (n_in + n_o) * 2, "resize_copy": (n_in + 3 * n_o) * 2},
                        reps, rounds, same))
    # the LayerNorm that writes its slice, against vx_layernorm_f16 and the copy of its result (the 1/4 map's rows, C 96)
    Cc = 96
    Mo = B * (S // 4) * (S // 4)
    x = G.dev(rng.standard_normal((Mo, Cc), dtype=np.float32).astype(np.float16))
    lw, lb = G.dev(np.ones(Cc, np.float32)), G.dev(np.zeros(Cc, np.float32))
    cat1, cat2, tmp = G.empty(Mo * 2 * Cc * 2), G.empty(Mo * 2 * Cc * 2), G.empty(Mo * Cc * 2)
    ne, ss, ds = (C.c_int64 * 4)(Cc, Mo, 1, 1), (C.c_int64 * 4)(1, Cc, 0, 0), (C.c_int64 * 4)(1, 2 * Cc, 0, 0)

    def ln_in_place():
        L.vx_check(api.vx_layernorm_pix_f16(x.ptr, lw.ptr, lb.ptr, cat1.ptr, 2 * Cc, Mo, Cc, C.c_float(1e-5), None))

    def ln_copy():
        L.vx_check(api.vx_layernorm_f16(x.ptr, lw.ptr, lb.ptr, tmp.ptr, Mo, Cc, C.c_float(1e-5), 0, 0, 0, None))
        L.vx_check(api.vx_copy_strided_f16(tmp.ptr, cat2.ptr, ne, ss, ds, C.c_float(1.0), None))

    ln_in_place(); ln_copy(); G.sync()
    d = np.abs(cat1.to_numpy(np.float16, (Mo, 2 * Cc)).astype(np.float32) - cat2.to_numpy(np.float16, (Mo, 2 * Cc)).astype(np.float32)).max()
    rows.append(compare(f"layer norm {S // 4}^2 x {Cc} into a concat (max |diff| {d:.2g})", {"in_place": ln_in_place, "norm_copy": ln_copy},
                        {"in_place": Mo * Cc * 4, "norm_copy": Mo * Cc * 8}, reps, rounds))
    G.release()
    return rows


def build(dev, path, cfg, S, batch, fused):
    g = GR.Graph(dev, GR.Weights(path))
    g.set_fused_models(fused)
    m = GR.ModelRef(g)
    image = g.input((3, S, S, batch), GR.F32, "image")
    GR.birefnet_precompute(m, (S, S), cfg.window_size)
    out = GR.birefnet_predict(m, image, cfg.window_size, cfg.depths, cfg.n_heads)
    return g, image, out


def network(batch, S, steps):
    cfg = dataclasses.replace(synth.SWIN_T, embed_dim=64, n_heads=(2, 4, 8, 16), image_size=S)  # (see the module's docstring: 96 does not plan)
    rec = {"size": S, "steps": steps, "batch_asked": batch}
    with tempfile.TemporaryDirectory() as td:
        path = synth.write_birefnet_gguf(Path(td) / "lite.gguf", cfg, seed=9)
        dev = vision.Device.init(vision.Backend.gpu)
        free = C.c_size_t()
        total = C.c_size_t()
        name, arch = C.create_string_buffer(128), C.create_string_buffer(64)
        L.vx_check(G.api().vx_device_info(0, name, 128, arch, 64, C.byref(total), C.byref(free), None))
        while batch > 1:  # the largest batch whose per-node arena (the larger one) fits half of the free memory
            plan = build(None, path, cfg, S, batch, False)[0]
            plan.allocate()
            if plan.summary()["arena_bytes"] < free.value // 2:
                break
            batch //= 2
        rec["batch"] = batch
        say(f"  {name.value.decode()} ({arch.value.decode()}): {free.value / 2**30:.0f} GiB free; batch {batch}" + ("" if batch == rec["batch_asked"] else f" (asked for {rec['batch_asked']}: the arena does not fit)"))
        x = np.random.default_rng(2).standard_normal((batch, S, S, 3)).astype(np.float32)
        masks = {}
        for fused in (True, False):
            g, image, out = build(dev, path, cfg, S, batch, fused)
            g.use_hip_graph(True)
            g.allocate()
            g.set(image, x)
            for _ in range(3):
                g.compute()
            t0 = time.perf_counter()
            for _ in range(steps):
                g.compute()
            dt = (time.perf_counter() - t0) / steps
            key = "fused" if fused else "per_node"
            s = g.summary()
            masks[fused] = g.get(out)
            rec[f"graph_{key}_launches"], rec[f"graph_{key}_arena_mb"] = s["launches"], round(s["arena_bytes"] / 2**20, 1)
            rec[f"graph_{key}_ms"], rec[f"graph_{key}_images_per_s"] = round(dt * 1e3, 3), round(batch / dt, 2)
            say(f"  graph-built, {key}: {s['launches']} launches, arena {rec[f'graph_{key}_arena_mb']} MiB, {rec[f'graph_{key}_ms']} ms per step = {rec[f'graph_{key}_images_per_s']} images / s")
            del g
        rec["fused_vs_per_node_max_abs"] = float(np.abs(masks[True] - masks[False]).max())
        say(f"  fused against per node, the masks: max abs difference {rec['fused_vs_per_node_max_abs']:.3g}")
        model = vision.Model.load(path, dev)
        imgs = synth.images(batch, S, S, seed=3)
        din, dout = vision.DeviceBuffer.from_numpy(imgs), vision.DeviceBuffer(batch * S * S * 4)
        run = lambda: model.segment_batch_device(din.ptr, batch, S, S, dout.ptr)  # noqa: E731
        for _ in range(3):
            run()
        G.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            run()
        G.sync()
        dt = (time.perf_counter() - t0) / steps
        rec["hand_step_ms"], rec["hand_images_per_s"] = round(dt * 1e3, 3), round(batch / dt, 2)
        say(f"  hand schedule (visp_birefnet_compute_batch_device: u8 in, its normalisation included; other work at the front end: no ratio): {rec['hand_step_ms']} ms per step = "
            f"{rec['hand_images_per_s']} images / s")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "birefnet_graph_bench.txt"))
    a = ap.parse_args()
    assert G.api().vx_device_count() > 0, "no HIP device visible: a timing needs the GPU"
    say(f"kernels of csrc/kernels_imgops.hip at batch {a.batch}, image {a.size}^2: device events around {a.reps} launches after 3 warm-up launches, {a.rounds} rounds; median us, spread = max - min "
        f"over rounds; byte bound at {HBM / 1e12} TB/s")
    kernels = kernel_cases(a.batch, a.size, a.reps, a.rounds)
    say(f"BiRefNet at {a.size}^2 on SWIN_T's depths at embed_dim 64: the graph-built birefnet_predict replayed as a hipGraph and the hand schedule's step (host clock around {a.steps} calls, 3 warm-up calls)")
    net = network(a.batch, a.size, a.steps)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("\n".join(RECORD) + "\n")
    print(json.dumps({"bench": "birefnet_graph", "reps": a.reps, "rounds": a.rounds, "kernels": kernels, "network": net}))


if __name__ == "__main__":
    main()
