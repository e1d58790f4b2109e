#!/usr/bin/env python3
"""usage: convert_yolov9t.py yolov9t_converted.pth [-o out.gguf] [--bn-eps 1e-3]   YOLOv9t torch state dict -> GGUF, see
vision.cpp_amd/convert.py (convert_yolov9t). The file is read with torch.load(weights_only=True); `model.22.*` and `detect.*` head
names are both accepted and every BatchNorm is folded into its conv with --bn-eps (1e-3 for ultralytics checkpoints)."""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from __graft_entry__ import load_package  # noqa: E402

load_package()
from visioncpp_amd import convert  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("input")
ap.add_argument("--output", "-o", default=None)
ap.add_argument("--bn-eps", type=float, default=1e-3)
a = ap.parse_args()
import torch  # noqa: E402

sd = torch.load(a.input, map_location="cpu", weights_only=True)
for wrap in ("state_dict", "model"):
    if isinstance(sd, dict) and wrap in sd and isinstance(sd[wrap], dict):
        sd = sd[wrap]
sd = {k: v.float().numpy() for k, v in sd.items() if hasattr(v, "numpy")}
out = a.output or str(Path(a.input).with_suffix("")) + "-F16.gguf"
print(convert.convert_yolov9t(sd, out, a.bn_eps))
