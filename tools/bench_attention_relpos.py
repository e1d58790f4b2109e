#!/usr/bin/env python3
"""Launch time of vx_attention_relpos_f16 (csrc/kernels_attn_relpos.hip) at the shapes of a SAM ViT-B image encoder, against two baselines on the same machine in
the same run. Prints a text record, writes it to --out (profiles/attn_relpos_bench.txt) and prints, last, one JSON line. A measurement, not a gate.

  * window shape: 14 x 14 tokens, 12 heads, 25 windows x 8 images. Baseline: vx_attention_masked_f16 fed the materialised bias [B, heads, T, T] f16, plus the
    time torch takes on the device to produce that bias the way transformers' get_decomposed_rel_pos does (two einsums and a broadcast add, f16).
  * global shape: 64 x 64 tokens, 12 heads, batch 1 and 8. Floor: vx_attention_f16, the bias-free head_dim-64 kernel, at T = 4096 (the bias cannot be
    materialised there: 403 MB per image).
Device events around `reps` back-to-back launches, `samples` such windows per kernel after warm-up launches, the kernels of a shape alternating; min / median /
max of the per-launch means. The achieved rate is the algorithm's 4 T^2 hd (+ 2 T (2 gw + 2 gh - 2) hd for the bias products) per (batch, head) over the median.

    python tools/bench_attention_relpos.py [--samples 20] [--reps 10] [--warmup 3] [--out profiles/attn_relpos_bench.txt]"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from tests import gpu_util as U  # noqa: E402
from visioncpp_amd import _lib as L  # noqa: E402

HD, HEADS = 64, 12
Q_SCALE = 0.18033688011112042  # VX_ATTN_Q_SCALE: log2(e) / sqrt(64), what the baselines' q is pre-scaled by


def stats(ts):
    return dict(min=round(float(min(ts)), 2), median=round(float(np.median(ts)), 2), max=round(float(max(ts)), 2))


def window_us(fn, reps):
    api = U.api()
    e0, e1 = C.c_void_p(), C.c_void_p()
    api.vx_event_create(C.byref(e0)); api.vx_event_create(C.byref(e1))
    api.vx_event_record(e0, None)
    for _ in range(reps):
        fn()
    api.vx_event_record(e1, None)
    U.sync()
    ms = C.c_float()
    api.vx_event_elapsed_ms(e0, e1, C.byref(ms))
    api.vx_event_destroy(e0); api.vx_event_destroy(e1)
    return ms.value / reps * 1e3


def alternate(a, fns):
    for _ in range(a.warmup):
        for fn in fns.values():
            fn()
    U.sync()
    ts = {name: [] for name in fns}
    for _ in range(a.samples):
        for name, fn in fns.items():
            ts[name].append(window_us(fn, a.reps))
    return {name: stats(t) for name, t in ts.items()}


def operands(gw, gh, B, seed):
    rng = np.random.default_rng(seed)
    T = gw * gh
    q, k, v = (rng.standard_normal((B, T, HEADS, HD)).astype(np.float16) for _ in range(3))
    rel_h, rel_w = ((rng.standard_normal((2 * g - 1, HD)) * 0.25).astype(np.float16) for g in (gh, gw))
    return q, k, v, rel_h, rel_w


def head_major(x, scale=1.0):
    return np.ascontiguousarray((x.astype(np.float32) * scale).astype(np.float16).transpose(0, 2, 1, 3))


def torch_bias_us(a, q, rel_h, rel_w, gw, gh):
    """-> (stats of the time torch takes on the device to make the [B, heads, T, T] f16 bias, the bias as numpy), or (a reason, None)"""
    try:
        import torch
        if not torch.cuda.is_available():
            return "not measured: torch sees no device", None
        dev = torch.device("cuda")
        B, T = q.shape[0], gw * gh
        tq = torch.from_numpy(head_major(q)).to(dev).reshape(B * HEADS, gh, gw, HD)
        iy, ix = torch.arange(gh, device=dev), torch.arange(gw, device=dev)
        Rh = torch.from_numpy(rel_h).to(dev)[(iy[:, None] - iy[None, :]) + gh - 1]
        Rw = torch.from_numpy(rel_w).to(dev)[(ix[:, None] - ix[None, :]) + gw - 1]

        def make():
            return (torch.einsum("bhwc,hkc->bhwk", tq, Rh)[:, :, :, :, None] + torch.einsum("bhwc,wkc->bhwk", tq, Rw)[:, :, :, None, :]).reshape(B, HEADS, T, T)

        for _ in range(a.warmup):
            make()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.samples):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                bias = make()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / a.reps * 1e3)
        return stats(ts), bias.cpu().numpy()
    except Exception as e:  # the baseline's second half is a courtesy: say why it is missing
        return f"not measured: {e}", None


def host_bias(q, rel_h, rel_w, gw, gh):
    """the [B, heads, T, T] f16 bias made with numpy on the host: what the masked baseline is fed where torch has no device (its content does not change the time)"""
    t = np.arange(gw * gh)
    y, x = t // gw, t % gw
    qh = q.astype(np.float32).transpose(0, 2, 1, 3)  # [B, heads, T, hd]
    ph = (qh @ rel_h.astype(np.float32).T)[:, :, t[:, None], y[:, None] - y[None, :] + gh - 1]
    pw = (qh @ rel_w.astype(np.float32).T)[:, :, t[:, None], x[:, None] - x[None, :] + gw - 1]
    return (ph + pw).astype(np.float16)


def flops(gw, gh, B, bias=True):
    T = gw * gh
    return B * HEADS * (4.0 * T * T * HD + (2.0 * T * (2 * gw + 2 * gh - 2) * HD if bias else 0.0))


def bench_window(a):
    api, gw, gh, B = U.api(), 14, 14, 25 * 8
    T = gw * gh
    q, k, v, rel_h, rel_w = operands(gw, gh, B, 1)
    d = [U.dev(x) for x in (q, k, v, rel_h, rel_w)]
    out, out_m = U.empty(B * T * HEADS * HD * 2), U.empty(B * T * HEADS * HD * 2)
    fns = {"relpos": lambda: L.vx_check(api.vx_attention_relpos_f16(*(b.ptr for b in d), out.ptr, B, HEADS, gw, gh, HD, 0.125, None))}
    tb, bias = torch_bias_us(a, q, rel_h, rel_w, gw, gh)
    if bias is None:
        bias = host_bias(q, rel_h, rel_w, gw, gh)
    if bias is not None:
        dq, dk, dv, dm = U.dev(head_major(q, Q_SCALE)), U.dev(head_major(k)), U.dev(head_major(v)), U.dev(np.ascontiguousarray(bias))
        fns["masked"] = lambda: L.vx_check(api.vx_attention_masked_f16(dq.ptr, dk.ptr, dv.ptr, dm.ptr, out_m.ptr, B, HEADS, T, HD, HEADS, B, 0, None))
    t = alternate(a, fns)
    row = dict(shape=f"window 14x14, {HEADS} heads, B = 25 x 8", relpos_us=t["relpos"], relpos_tflops=round(flops(gw, gh, B) / t["relpos"]["median"] * 1e-6, 1),
               masked_us=t.get("masked", "not measured"), torch_bias_us=tb, bias_bytes=B * HEADS * T * T * 2)
    if bias is not None:
        ya, yb = (b.to_numpy(np.float16, (B * T, HEADS * HD)).astype(np.float32) for b in (out, out_m))
        row["outputs_differ_by"] = float(f"{np.abs(ya - yb).max() / np.abs(yb).max():.3g}")
    return row


def bench_global(a, B):
    api, gw, gh = U.api(), 64, 64
    T = gw * gh
    q, k, v, rel_h, rel_w = operands(gw, gh, B, 2)
    d = [U.dev(x) for x in (q, k, v, rel_h, rel_w)]
    dq, dk, dv = U.dev(head_major(q, Q_SCALE)), U.dev(head_major(k)), U.dev(head_major(v))
    out, out_f = U.empty(B * T * HEADS * HD * 2), U.empty(B * T * HEADS * HD * 2)
    t = alternate(a, {"relpos": lambda: L.vx_check(api.vx_attention_relpos_f16(*(b.ptr for b in d), out.ptr, B, HEADS, gw, gh, HD, 0.125, None)),
                      "floor": lambda: L.vx_check(api.vx_attention_f16(dq.ptr, dk.ptr, dv.ptr, out_f.ptr, B, HEADS, T, None))})
    return dict(shape=f"global 64x64, {HEADS} heads, B = {B}", relpos_us=t["relpos"], relpos_tflops=round(flops(gw, gh, B) / t["relpos"]["median"] * 1e-6, 1),
                floor_us=t["floor"], floor_tflops=round(flops(gw, gh, B, False) / t["floor"]["median"] * 1e-6, 1),
                bias_share_of_flops=round(1.0 - flops(gw, gh, B, False) / flops(gw, gh, B), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attn_relpos_bench.txt"))
    a = ap.parse_args()
    assert U.api().vx_device_count() > 0, "no HIP device visible: there is nothing to measure without one"
    L.vx_check(U.api().vx_set_device(0))
    rows = [bench_window(a)]
    U.release()
    for B in (1, 8):
        rows.append(bench_global(a, B))
        U.release()
    lines = [f"vx_attention_relpos_f16 on the MI355X; {a.samples} samples of {a.reps} launches after {a.warmup} warm-up rounds; us per launch, min / median / max"]
    for r in rows:
        lines.append(r["shape"] + ": " + ", ".join(f"{k} {v}" for k, v in r.items() if k != "shape"))
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).write_text(text)
    print(json.dumps(dict(tool="bench_attention_relpos", samples=a.samples, reps=a.reps, rows=rows)))


if __name__ == "__main__":
    main()
