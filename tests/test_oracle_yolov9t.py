"""The numpy restatement tests/yolov9t_ref.py against an independent torch.nn.functional statement of ultralytics' YOLOv9t
modules (Conv with BatchNorm, RepConv with two branches, RepNCSPELAN4, AConv, SPPELAN, Detect with DFL) run on the UNFUSED synthetic
checkpoint (BatchNorm present, head under model.22.), so that the converter's BatchNorm folding and renaming are checked as well."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import yolov9t_ref  # noqa: E402
from visioncpp_amd import convert, synth  # noqa: E402

torch = pytest.importorskip("torch")
F = torch.nn.functional
EPS = 1e-3


def _torch_forward(sd, x):
    """x [B, 3, S, S] float64 -> boxes [B, A, 4], scores [B, A, nc]."""
    T = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items() if v.dtype != np.int64}

    def conv(p, x, s=1, act=True):  # Conv: conv (no bias) + BatchNorm + SiLU
        w = T[p + ".conv.weight"]
        y = F.conv2d(x, w, None, s, w.shape[-1] // 2)
        y = F.batch_norm(y, T[p + ".bn.running_mean"], T[p + ".bn.running_var"], T[p + ".bn.weight"], T[p + ".bn.bias"], False, 0.0, EPS)
        return F.silu(y) if act else y

    def repcsp(p, x):
        a, b = conv(p + ".cv1", x), conv(p + ".cv2", x)
        for j in range(3):
            q = f"{p}.m.{j}"
            a = a + conv(q + ".cv2", F.silu(conv(q + ".cv1.conv1", a, act=False) + conv(q + ".cv1.conv2", a, act=False)))
        return conv(p + ".cv3", torch.cat([a, b], 1))

    def elan4(p, x):
        y = list(conv(p + ".cv1", x).chunk(2, 1))
        y.append(conv(p + ".cv2.1", repcsp(p + ".cv2.0", y[-1])))
        y.append(conv(p + ".cv3.1", repcsp(p + ".cv3.0", y[-1])))
        return conv(p + ".cv4", torch.cat(y, 1))

    def aconv(p, x):
        return conv(p + ".cv1", F.avg_pool2d(x, 2, 1, 0, False, True), 2)

    f = {0: conv("model.0", x, 2)}
    f[1] = conv("model.1", f[0], 2)
    y = list(conv("model.2.cv1", f[1]).chunk(2, 1))
    y.append(conv("model.2.cv2", y[-1]))
    y.append(conv("model.2.cv3", y[-1]))
    f[2] = conv("model.2.cv4", torch.cat(y, 1))
    f[3] = aconv("model.3", f[2])
    f[4] = elan4("model.4", f[3])
    f[5] = aconv("model.5", f[4])
    f[6] = elan4("model.6", f[5])
    f[7] = aconv("model.7", f[6])
    f[8] = elan4("model.8", f[7])
    y = [conv("model.9.cv1", f[8])]
    for _ in range(3):
        y.append(F.max_pool2d(y[-1], 5, 1, 2))
    f[9] = conv("model.9.cv5", torch.cat(y, 1))
    up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")  # noqa: E731
    f[12] = elan4("model.12", torch.cat([up(f[9]), f[6]], 1))
    f[15] = elan4("model.15", torch.cat([up(f[12]), f[4]], 1))
    f[18] = elan4("model.18", torch.cat([aconv("model.16", f[15]), f[12]], 1))
    f[21] = elan4("model.21", torch.cat([aconv("model.19", f[18]), f[9]], 1))
    outs, anchors, strides = [], [], []
    for lv, xl in enumerate((f[15], f[18], f[21])):
        h = "model.22"
        r = conv(f"{h}.cv2.{lv}.1", conv(f"{h}.cv2.{lv}.0", xl))
        r = F.conv2d(r, T[f"{h}.cv2.{lv}.2.weight"], T[f"{h}.cv2.{lv}.2.bias"])
        c = conv(f"{h}.cv3.{lv}.1", conv(f"{h}.cv3.{lv}.0", xl))
        c = F.conv2d(c, T[f"{h}.cv3.{lv}.2.weight"], T[f"{h}.cv3.{lv}.2.bias"])
        B, _, hh, ww = r.shape
        outs.append(torch.cat([r, c], 1).view(B, -1, hh * ww))
        sy, sx = torch.meshgrid(torch.arange(hh, dtype=torch.float64) + 0.5, torch.arange(ww, dtype=torch.float64) + 0.5, indexing="ij")
        anchors.append(torch.stack([sx, sy], -1).view(-1, 2))
        strides.append(torch.full((hh * ww, 1), 8.0 * 2 ** lv, dtype=torch.float64))
    xc = torch.cat(outs, 2)
    B = xc.shape[0]
    box, cls = xc[:, :64], xc[:, 64:]
    proj = T["model.22.dfl.conv.weight"].view(1, 16, 1, 1)
    dist = (box.view(B, 4, 16, -1).transpose(2, 1).softmax(1) * proj).sum(1)  # DFL: [B, 4, A]
    anc, st = torch.cat(anchors).T[None], torch.cat(strides).T[None]
    lt, rb = dist.chunk(2, 1)
    boxes = torch.cat([anc - lt, anc + rb], 1) * st
    return boxes.transpose(1, 2).numpy(), cls.sigmoid().transpose(1, 2).numpy()


def test_oracle_matches_torch_statement_of_the_unfused_checkpoint():
    raw_sd = synth.yolov9t_state_dict(seed=5, fused=False, head_prefix="model.22.")
    assert any(".bn.running_var" in k for k in raw_sd) and "model.22.cv3.0.2.weight" in raw_sd
    folded = convert.fold_yolov9t(raw_sd, 1e-3)
    assert not any(".bn." in k or k.startswith("model.22.") or ".dfl." in k for k in folded)
    assert folded.keys() == synth.yolov9t_state_dict(seed=5).keys()
    x = synth.images(2, 128, 128, seed=9).astype(np.float32) / 255.0
    boxes, scores = yolov9t_ref.forward(folded, x)
    tb, ts = _torch_forward(raw_sd, torch.from_numpy(x.transpose(0, 3, 1, 2).astype(np.float64)))
    assert boxes.shape == tb.shape == (2, 16 * 16 + 8 * 8 + 4 * 4, 4) and scores.shape == ts.shape == (2, 336, 80)
    assert np.abs(boxes - tb).max() <= 1e-4 * np.abs(tb).max()
    assert np.abs(scores - ts).max() <= 1e-4
    assert ts.std() > 1e-2 and np.abs(tb).max() > 10  # the synthetic weights produce varied outputs


def test_converter_writes_the_file_contract(tmp_path):
    from visioncpp_amd.gguf import GGUFFile

    sd = synth.yolov9t_state_dict(seed=1, fused=False, head_prefix="model.22.")
    path = convert.convert_yolov9t(sd, tmp_path / "y.gguf")
    f = GGUFFile(path)
    assert f.kv["general.architecture"] == "yolov9t" and f.kv["yolov9t.tensor_data_layout"] == "whcn"
    names = f.tensor_names
    assert "detect.cv3.0.2.weight" in names and "model.4.cv2.0.m.2.cv1.conv2.conv.bias" in names
    listed = {names[i] for i in f.kv["yolov9t.conv2d_weights"]}
    assert listed == {n for n in names if n.endswith(".weight")}
    with pytest.raises(ValueError):
        convert.convert_yolov9t({"model.0.conv.weight": np.zeros((16, 3, 3, 3), np.float32)}, tmp_path / "bad.gguf")
