"""Python face of the backend: the reference's bindings/python/visioncpp/vision.py classes
(Backend, Device, Arch, Model.load/compute) on top of the same C symbols, plus the batched
extension (`Model.compute_batch`, device-resident `compute_batch_device`)."""
from __future__ import annotations

import ctypes
from ctypes import byref, c_int32, c_int64, c_size_t, c_void_p
from enum import Enum
from pathlib import Path

import numpy as np

from . import _lib as lib
from ._lib import check, get_lib, vx_check


class ImageFormat(Enum):
    rgba_u8 = 0
    bgra_u8 = 1
    argb_u8 = 2
    rgb_u8 = 3
    alpha_u8 = 4
    rgba_f32 = 5
    rgb_f32 = 6
    alpha_f32 = 7


class Backend(Enum):
    auto = 0
    cpu = 1
    gpu = 2
    vulkan = gpu | 1 << 8


class Arch(Enum):
    sam = 0
    birefnet = 1
    depth_anything = 2
    migan = 3
    esrgan = 4
    unknown = 5


class Device:
    @staticmethod
    def init(backend: Backend = Backend.auto, index: int | None = None):
        api = get_lib()
        handle = c_void_p()
        if index is None:
            check(api.visp_device_init(backend.value, byref(handle)))
        else:
            check(api.visp_hip_device_init(index, byref(handle)))
        return Device(api, handle)

    def __init__(self, api, handle):
        self._api, self._handle = api, handle

    @property
    def type(self) -> Backend:
        return Backend(self._api.visp_device_type(self._handle))

    @property
    def name(self) -> str:
        return self._api.visp_device_name(self._handle).decode()

    @property
    def description(self) -> str:
        return self._api.visp_device_description(self._handle).decode()

    def __del__(self):
        if getattr(self, "_handle", None):
            self._api.visp_device_destroy(self._handle)
            self._handle = None


_CHANNELS = {0: 4, 1: 4, 2: 4, 3: 3, 4: 1, 5: 4, 6: 3, 7: 1}


class Model:
    @classmethod
    def load(cls, path, device: Device, arch: Arch = Arch.unknown, no_upload: bool = False):
        api = get_lib()
        handle = c_void_p()
        p = lib.path_to_char_p(path)
        if arch is Arch.unknown:
            v = c_int32()
            check(api.visp_model_detect_family(p, byref(v)))
            arch = Arch(v.value)
        check(api.visp_model_load_ex(p, device._handle, arch.value, 1 if no_upload else 0, byref(handle)))
        return cls(api, handle, arch, device)

    def __init__(self, api, handle, arch: Arch, device: Device):
        self.arch, self._api, self._handle, self._device = arch, api, handle, device

    def __del__(self):
        if getattr(self, "_handle", None):
            self._api.visp_model_destroy(self._handle, self.arch.value)
            self._handle = None

    # ---- reference API: one image of any size/format -> u8 depth map (c-api.cpp:230-251)
    def compute(self, image: np.ndarray, format: ImageFormat = ImageFormat.rgb_u8, args: list[int] | None = None) -> np.ndarray:
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape[:2]
        view = lib.ImageView(w, h, w * _CHANNELS[format.value], format.value, img.ctypes.data)
        views = (lib.ImageView * 1)(view)
        out_view, out_data = lib.ImageView(), c_void_p()
        a = list(args or [])
        check(self._api.visp_model_compute(self._handle, self.arch.value, views, 1, (c_int32 * max(1, len(a)))(*a), len(a), byref(out_view), byref(out_data)))
        return self._take_image(out_view, out_data)

    def _take_image(self, out_view, out_data) -> np.ndarray:
        try:
            n = out_view.height * out_view.stride
            buf = (ctypes.c_uint8 * n).from_address(out_view.data)
            ch = out_view.stride // max(1, out_view.width)
            res = np.frombuffer(buf, np.uint8).reshape(out_view.height, out_view.width, ch).copy()
            if ch == 1:
                res = res[..., 0]
        finally:
            self._api.visp_image_destroy(out_data)
        return res

    def _family_fn(self, name: str):
        prefix = {Arch.esrgan: "visp_esrgan_", Arch.sam: "visp_sam_", Arch.birefnet: "visp_swin_", Arch.migan: "visp_migan_"}.get(self.arch, "visp_depthany_")
        return getattr(self._api, prefix + name)

    # ---- batched extension
    @property
    def info(self) -> lib.DepthAnyInfo:
        i = lib.DepthAnyInfo()
        check(self._api.visp_depthany_get_info(self._handle, byref(i)))
        return i

    def image_extent(self, w: int, h: int):
        ow, oh = c_int32(), c_int32()
        check(self._api.visp_depthany_image_extent(self._handle, w, h, byref(ow), byref(oh)))
        return ow.value, oh.value

    def weights_arena(self):
        p, n = c_void_p(), c_size_t()
        check(self._family_fn("weights_arena")(self._handle, byref(p), byref(n)))
        return p.value, n.value

    def weights_ready(self):
        check(self._family_fn("weights_ready")(self._handle))

    def reserve(self, batch: int, w: int, h: int):
        check(self._api.visp_depthany_reserve(self._handle, batch, w, h))

    def use_graph(self, enable: bool = True):
        check(self._api.visp_depthany_use_graph(self._handle, int(enable)))

    def sam_set_fp8_mlp(self, enable: bool = True):
        """MobileSAM encoder, opt-in: the transformer stages' MLPs on the e4m3 matrix instruction (BASELINE.json configs[4]); several percent of
        embedding error (tests/test_fp8_decision.py rejected it for masks). Never the default."""
        check(self._api.visp_sam_set_fp8_mlp(self._handle, int(enable)))

    def set_schedule(self, schedule: int):
        """-1 = automatic (the default: the token-stationary block kernel where the model has its shape, embed dim 384 / mlp 1536 /
        head dim 64, otherwise GEMM launches); 0 = GEMM launches per op group; 1 = block kernel per layer."""
        check(self._api.visp_depthany_set_schedule(self._handle, int(schedule)))

    def set_split(self, n: int):
        """Sub-batches of one step on parallel streams: 0 = automatic, 1 = none, up to 4 (bit-identical results)."""
        check(self._api.visp_depthany_set_split(self._handle, int(n)))

    def compute_batch(self, images: np.ndarray, return_raw: bool = False):
        """images: uint8 [B, h, w, 3] on the host -> float32 [B, h, w] in [0, 1]."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert c == 3
        out = np.empty((b, h, w), np.float32)
        raw = np.empty((b, h, w), np.float32) if return_raw else None
        check(self._api.visp_depthany_compute_batch_host(self._handle, imgs.ctypes.data, b, w, h, out.ctypes.data,
                                                         raw.ctypes.data if return_raw else None))
        return (out, raw) if return_raw else out

    def compute_batch_device(self, rgb_dev: int, batch: int, w: int, h: int, out_dev: int, raw_dev: int | None = None,
                             stream: int | None = None):
        check(self._api.visp_depthany_compute_batch_device(self._handle, rgb_dev, batch, w, h, out_dev, raw_dev, stream))

    def compute_scaled_batch(self, images: np.ndarray) -> np.ndarray:
        """images: uint8 [B, h, w, 3] of ANY extent on the host -> float32 [B, h, w] in [0, 1]: depthany_compute per image, scaled on the device."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert c == 3
        out = np.empty((b, h, w), np.float32)
        check(self._api.visp_depthany_compute_scaled_batch_host(self._handle, imgs.ctypes.data, b, w, h, out.ctypes.data))
        return out

    def compute_scaled_batch_device(self, rgb_dev: int, batch: int, w: int, h: int, out_dev: int, stream: int | None = None):
        """The same on device-resident arrays (addresses): rgb_u8 [batch, h, w, 3] -> f32 [batch, h, w]; nothing leaves the device."""
        check(self._api.visp_depthany_compute_scaled_batch_device(self._handle, rgb_dev, batch, w, h, out_dev, stream))

    def enable_captures(self, enable: bool = True):
        check(self._family_fn("enable_captures")(self._handle, int(enable)))

    def read_capture(self, name: str) -> np.ndarray:
        n, shape = c_int64(), (c_int64 * 4)()
        f = self._family_fn("read_capture")
        check(f(self._handle, name.encode(), None, 0, byref(n), shape))
        out = np.empty(n.value, np.float32)
        check(f(self._handle, name.encode(), out.ctypes.data, n.value, byref(n), shape))
        dims = [int(d) for d in shape]
        while len(dims) > 1 and dims[-1] == 1:
            dims.pop()
        return out.reshape(dims)

    def enable_timing(self, enable: bool = True):
        check(self._family_fn("enable_timing")(self._handle, int(enable)))

    def read_timing(self):
        arr, n = (lib.Timing * 256)(), c_int32()
        check(self._family_fn("read_timing")(self._handle, arr, 256, byref(n)))
        return [dict(name=arr[i].name.decode(), ms=arr[i].ms, launches=arr[i].launches, flops=arr[i].flops, bytes=arr[i].bytes)
                for i in range(n.value)]


    # ---- BiRefNet (family 1): batched extension
    def swin_set_mask_mode(self, shifted_only: bool):
        """False (default) = the reference as written: the layer's shift mask acts in every block (swin.cpp:128-139, 226-237);
        True = shifted blocks only, as the reference's torch twin / the original Swin."""
        check(self._api.visp_swin_set_mask_mode(self._handle, int(bool(shifted_only))))

    def birefnet_image_extent(self, w: int, h: int):
        ow, oh = c_int32(), c_int32()
        check(self._api.visp_birefnet_image_extent(self._handle, w, h, byref(ow), byref(oh)))
        return ow.value, oh.value

    def segment_batch(self, images: np.ndarray) -> np.ndarray:
        """images: uint8 [B, h, w, 3] at the model extent -> sigmoid masks f32 [B, h, w] (birefnet_predict per image)."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert c == 3
        out = np.empty((b, h, w), np.float32)
        check(self._api.visp_birefnet_compute_batch_host(self._handle, imgs.ctypes.data, b, w, h, out.ctypes.data))
        return out

    def segment_batch_device(self, rgb_dev: int, batch: int, w: int, h: int, mask_dev: int, stream: int | None = None):
        check(self._api.visp_birefnet_compute_batch_device(self._handle, rgb_dev, batch, w, h, mask_dev, stream))

    def birefnet_cutout_batch(self, images: np.ndarray, radius: int = 30) -> np.ndarray:
        """images: uint8 [B, h, w, 3] at the model extent -> uint8 [B, h, w, 4]: foreground colours from the estimator on the network's mask, alpha = the mask."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert c == 3
        out = np.empty((b, h, w, 4), np.uint8)
        check(self._api.visp_birefnet_cutout_batch_host(self._handle, imgs.ctypes.data, b, w, h, int(radius), out.ctypes.data))
        return out

    def birefnet_cutout_batch_device(self, rgb_dev: int, batch: int, w: int, h: int, rgba_dev: int, radius: int = 30, stream: int | None = None):
        check(self._api.visp_birefnet_cutout_batch_device(self._handle, rgb_dev, batch, w, h, int(radius), rgba_dev, stream))

    def birefnet_cutout(self, image: np.ndarray, format: ImageFormat = ImageFormat.rgb_u8, radius: int = 30) -> np.ndarray:
        """One 8-bit colour image of any extent -> uint8 [h, w, 4] cutout at that extent."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape[:2]
        view = lib.ImageView(w, h, w * _CHANNELS[format.value], format.value, img.ctypes.data)
        out_view, out_data = lib.ImageView(), c_void_p()
        check(self._api.visp_birefnet_cutout(self._handle, byref(view), int(radius), byref(out_view), byref(out_data)))
        return self._take_image(out_view, out_data)

    # ---- ESRGAN (family 4): batched extension
    @property
    def esrgan_info(self) -> lib.EsrganInfo:
        i = lib.EsrganInfo()
        check(self._api.visp_esrgan_get_info(self._handle, byref(i)))
        return i

    def set_tile_group(self, tiles: int):
        check(self._api.visp_esrgan_set_tile_group(self._handle, tiles))

    def upscale_batch(self, images: np.ndarray, format: ImageFormat = ImageFormat.rgb_u8) -> np.ndarray:
        """images: uint8 [B, h, w, C] on the host -> rgba uint8 [B, h*scale, w*scale, 4] (esrgan_compute per image)."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert c == _CHANNELS[format.value]
        s = self.esrgan_info.scale
        out = np.empty((b, h * s, w * s, 4), np.uint8)
        check(self._api.visp_esrgan_compute_batch_host(self._handle, imgs.ctypes.data, b, w, h, format.value, out.ctypes.data))
        return out

    def upscale_batch_device(self, img_dev: int, batch: int, w: int, h: int, out_dev: int, format: ImageFormat = ImageFormat.rgb_u8,
                             stream: int | None = None):
        check(self._api.visp_esrgan_compute_batch_device(self._handle, img_dev, batch, w, h, format.value, out_dev, stream))

    def esrgan_generate(self, tiles: np.ndarray) -> np.ndarray:
        """rgb float32 tiles [n, h, w, 3] -> [n, h*scale, w*scale, 3] (esrgan_generate, no tiling / u8 conversion)."""
        t = np.ascontiguousarray(tiles, dtype=np.float32)
        n, h, w, c = t.shape
        assert c == 3
        s = self.esrgan_info.scale
        out = np.empty((n, h * s, w * s, 3), np.float32)
        check(self._api.visp_esrgan_generate_host(self._handle, t.ctypes.data, n, w, h, out.ctypes.data))
        return out

    # ---- MobileSAM image encoder (family 0)
    def sam_encode(self, image: np.ndarray, format: ImageFormat = ImageFormat.rgb_u8) -> np.ndarray:
        """sam_encode (reference vision.cpp:36-52): one u8 colour image of any extent -> embedding float32 [64, 64, 256]."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        h, w = img.shape[:2]
        view = lib.ImageView(w, h, w * _CHANNELS[format.value], format.value, img.ctypes.data)
        check(self._api.visp_sam_encode(self._handle, byref(view)))
        shape = (c_int64 * 3)()
        out = np.empty((64, 64, 256), np.float32)
        check(self._api.visp_sam_read_embedding(self._handle, out.ctypes.data, out.size, shape))
        return out.reshape([int(d) for d in shape])

    def sam_compute(self, prompt: list[int]) -> np.ndarray:
        """sam_compute (reference vision.cpp:54-92) on the last sam_encode: point [x, y] or box [x0, y0, x1, y1] -> u8 mask [h, w]."""
        out_view, out_data = lib.ImageView(), c_void_p()
        check(self._api.visp_sam_compute(self._handle, (c_int32 * len(prompt))(*prompt), len(prompt), byref(out_view), byref(out_data)))
        return self._take_image(out_view, out_data)

    def sam_read_masks(self):
        """mask logits [4, 256, 256] and iou predictions [4] of the last sam_compute."""
        masks, iou = np.empty((4, 256, 256), np.float32), (ctypes.c_float * 4)()
        check(self._api.visp_sam_read_masks(self._handle, masks.ctypes.data, masks.size, iou))
        return masks, np.array(list(iou), np.float32)

    # ---- many prompts per sam_encode in one batched pass
    @staticmethod
    def _sam_prompt_arrays(prompts):
        """[[x, y] | [x0, y0, x1, y1], ..] -> (int32 [n, 4], int32 [n]); a count other than 2 or 4 is passed on for the library to refuse"""
        p = np.zeros((len(prompts), 4), np.int32)
        k = np.zeros(len(prompts), np.int32)
        for i, q in enumerate(prompts):
            q = [int(v) for v in q]
            k[i] = len(q)
            p[i, : min(4, len(q))] = q[:4]
        return p, k

    def sam_image_extent(self):
        """(width, height) of the image given to the last sam_encode."""
        w, h = c_int32(), c_int32()
        check(self._api.visp_sam_image_extent(self._handle, byref(w), byref(h)))
        return w.value, h.value

    def sam_compute_batch(self, prompts):
        """prompts: points [x, y] and boxes [x0, y0, x1, y1], mixed as they come, on the last sam_encode ->
        (masks uint8 [n, h, w] of 0 / 255, iou float32 [n, 4], chosen int32 [n] = best of the first three masks by predicted iou)."""
        p, k = self._sam_prompt_arrays(prompts)
        n = len(prompts)
        w, h = self.sam_image_extent() if n else (0, 0)
        masks, iou, chosen = np.empty((n, h, w), np.uint8), np.empty((n, 4), np.float32), np.empty(n, np.int32)
        check(self._api.visp_sam_compute_batch_host(self._handle, p.ctypes.data, k.ctypes.data, n, masks.ctypes.data, iou.ctypes.data, chosen.ctypes.data))
        self._sam_batch_n = n
        return masks, iou, chosen

    def sam_compute_batch_device(self, prompts, masks_dev: int, iou_dev: int | None = None, chosen_dev: int | None = None, stream: int | None = None):
        """The same with device outputs (addresses): masks u8 [n, h, w], iou f32 [n, 4] and chosen i32 [n], the last two optional. Nothing waits for the
        device when a stream is given."""
        p, k = self._sam_prompt_arrays(prompts)
        check(self._api.visp_sam_compute_batch_device(self._handle, p.ctypes.data, k.ctypes.data, len(prompts), masks_dev, iou_dev, chosen_dev, stream))
        self._sam_batch_n = len(prompts)

    # ---- SAM's SamPredictor.predict: labelled points, a box with points, the previous low-resolution logits as mask input
    def sam_mask_input_size(self) -> int:
        """side of a mask input (256), 0 when the file has no prompt_encoder.mask_downscaling tensors"""
        s = c_int32()
        check(self._api.visp_sam_mask_input_size(self._handle, byref(s)))
        return s.value

    @staticmethod
    def _sam_predict_arrays(points, labels, box, mask_input):
        """one prompt (points [k, 2], box [4], mask_input [S, S]) or a batch of one shape ([n, k, 2], [n, 4], [n, S, S]) -> batch arrays, and whether it was one"""
        pts = np.zeros((0, 0, 2), np.int32) if points is None else np.ascontiguousarray(points, np.int32)
        bx = None if box is None else np.ascontiguousarray(box, np.int32)
        one = pts.ndim == 2 if points is not None else (bx is not None and bx.ndim == 1)
        if one:
            pts = pts[None] if points is not None else pts
            bx = None if bx is None else bx[None]
        n = pts.shape[0] if points is not None else (0 if bx is None else bx.shape[0])
        pts = pts.reshape(n, -1, 2)
        k = pts.shape[1]
        lab = np.ones((n, k), np.int32) if labels is None else np.ascontiguousarray(labels, np.int32).reshape(n, k)
        mi = None
        if mask_input is not None:
            mi = np.ascontiguousarray(mask_input, np.float32)
            mi = mi[None] if mi.ndim == 2 else mi
            if mi.ndim != 3 or mi.shape[0] != n or mi.shape[1] != mi.shape[2]:
                raise ValueError(f"mask_input of shape {mi.shape} for {n} prompts: expected [n, S, S]")
        if bx is not None and bx.shape != (n, 4):
            raise ValueError(f"box of shape {bx.shape} for {n} prompts: expected [n, 4]")
        return pts, lab, k, bx, mi, n, one

    def sam_predict(self, points, labels=None, box=None, mask_input=None, plane: int = -1):
        """SamPredictor.predict on the last sam_encode: points [k, 2] in image pixels with labels [k] (1 positive, the default; 0 negative; -1 not a point), an
        optional box [x0, y0, x1, y1] and an optional mask_input [S, S] (the low_res_logits of an earlier call) -- or a batch of prompts of one shape, every
        array with a leading n. plane -1: the best of the first three masks by predicted iou; 0 .. 3: that one (SAM's single-mask output is 0).
        -> (masks uint8 [h, w] of 0 / 255, iou float32 [4], chosen int, low_res_logits float32 [S, S]), each with a leading n for a batch."""
        pts, lab, k, bx, mi, n, one = self._sam_predict_arrays(points, labels, box, mask_input)
        w, h = self.sam_image_extent() if n else (0, 0)
        S = 4 * 64
        masks, iou, chosen, low = np.empty((n, h, w), np.uint8), np.empty((n, 4), np.float32), np.empty(n, np.int32), np.empty((n, S, S), np.float32)
        check(self._api.visp_sam_predict_host(self._handle, pts.ctypes.data if k else None, lab.ctypes.data if k else None, k, None if bx is None else bx.ctypes.data,
                                              None if mi is None else mi.ctypes.data, 0 if mi is None else mi.shape[1], n, int(plane), masks.ctypes.data, iou.ctypes.data,
                                              chosen.ctypes.data, low.ctypes.data))
        self._sam_batch_n = n
        return (masks[0], iou[0], int(chosen[0]), low[0]) if one else (masks, iou, chosen, low)

    def sam_predict_device(self, points, labels=None, box=None, mask_input_dev: int | None = None, plane: int = -1, *, masks_dev: int, iou_dev: int | None = None,
                           chosen_dev: int | None = None, low_res_dev: int | None = None, stream: int | None = None):
        """The same with the mask input and the outputs as device addresses (mask_input_dev f32 [n, S, S]; masks u8 [n, h, w], iou f32 [n, 4], chosen i32 [n],
        low_res f32 [n, S, S], the last three optional). Nothing waits for the device inside a chunk, or at all when a stream is given."""
        pts, lab, k, bx, _, n, _ = self._sam_predict_arrays(points, labels, box, None)
        check(self._api.visp_sam_predict_device(self._handle, pts.ctypes.data if k else None, lab.ctypes.data if k else None, k, None if bx is None else bx.ctypes.data,
                                                mask_input_dev, 4 * 64 if mask_input_dev else 0, n, int(plane), masks_dev, iou_dev, chosen_dev, low_res_dev, stream))
        self._sam_batch_n = n

    def sam_set_prompt_chunk(self, n: int):
        """Prompts per internal chunk of the batch calls (1 .. 256, default 64): sizes the workspace, about 27 MB per prompt in flight."""
        check(self._api.visp_sam_set_prompt_chunk(self._handle, int(n)))

    def sam_read_masks_batch(self):
        """mask logits [n, 4, 256, 256] and iou predictions [n, 4] of the last batch call (captures enabled)."""
        n = getattr(self, "_sam_batch_n", 0)
        masks, iou = np.empty((max(n, 1), 4, 256, 256), np.float32), np.empty((max(n, 1), 4), np.float32)
        check(self._api.visp_sam_read_masks_batch(self._handle, masks.ctypes.data, masks.size, iou.ctypes.data))
        return masks[:n], iou[:n]

    # ---- automatic mask generation: SAM's automatic mask generator on a prompt grid, selected on the device
    def _sam_generate_args(self, prompts, points_per_side, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh):
        if prompts is None:
            w, h = self.sam_image_extent()
            prompts = sam_point_grid(int(points_per_side), w, h)
        d = sam_generate_defaults()
        given = (pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh)
        params = [float(d[k]) if v is None else float(v) for k, v in zip(("pred_iou_thresh", "stability_thresh", "stability_offset", "nms_iou_thresh"), given)]
        p, k = self._sam_prompt_arrays(prompts)
        return p, k, params

    def sam_generate_masks_raw(self, prompts=None, points_per_side: int = 32, pred_iou_thresh=None, stability_thresh=None, stability_offset=None, nms_iou_thresh=None,
                               max_masks: int = 256, min_mask_region_area: int = 0):
        """The arrays of visp_sam_generate_masks_host, cut to the masks returned: (masks uint8 [k, h, w] of 0 / 255, info_i32 [k, 8] = {prompt, plane, x, y, w, h,
        area, 0}, info_f32 [k, 2] = {predicted_iou, stability_score}, counts (returned, kept before the cut to max_masks)).
        min_mask_region_area > 0 (visp_sam_generate_masks_clean_host): holes and islands below that many pixels are removed on the device and a second NMS runs,
        as SAM's postprocess_small_regions does; the masks then come in SAM's order, unchanged ones first and changed ones behind them, each by predicted iou --
        not the order without cleaning --, info_i32 column 7 is 1 for a changed mask and counts is (returned, kept by the first NMS, returned masks that
        cleaning changed, masks the second NMS removed)."""
        p, k, params = self._sam_generate_args(prompts, points_per_side, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh)
        n, cap = len(k), int(max_masks)
        w, h = self.sam_image_extent() if n and cap > 0 else (0, 0)
        masks, ii, fi = np.empty((max(cap, 0), h, w), np.uint8), np.empty((max(cap, 0), 8), np.int32), np.empty((max(cap, 0), 2), np.float32)
        area = int(min_mask_region_area)
        counts = np.zeros(4 if area else 2, np.int32)
        if area:
            check(self._api.visp_sam_generate_masks_clean_host(self._handle, p.ctypes.data, k.ctypes.data, n, *params, cap, area, masks.ctypes.data, ii.ctypes.data,
                                                               fi.ctypes.data, counts.ctypes.data))
        else:
            check(self._api.visp_sam_generate_masks_host(self._handle, p.ctypes.data, k.ctypes.data, n, *params, cap, masks.ctypes.data, ii.ctypes.data, fi.ctypes.data,
                                                         counts.ctypes.data))
        self._sam_batch_n = n
        r = int(counts[0])
        return masks[:r], ii[:r], fi[:r], (r, *(int(c) for c in counts[1:]))

    def sam_generate_masks_rle_raw(self, prompts=None, points_per_side: int = 32, pred_iou_thresh=None, stability_thresh=None, stability_offset=None, nms_iou_thresh=None,
                                   max_masks: int = 256, min_mask_region_area: int = 0):
        """sam_generate_masks_raw with RLE dicts (mask_to_rle's) in place of the mask array (visp_sam_generate_masks_rle_host): the masks are encoded on the
        device behind the generate call and no mask byte is read back. counts always has four entries; the last two are 0 without min_mask_region_area."""
        p, k, params = self._sam_generate_args(prompts, points_per_side, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh)
        n, cap = len(k), int(max_masks)
        w, h = self.sam_image_extent() if n and cap > 0 else (0, 0)
        ii, fi, counts = np.empty((max(cap, 0), 8), np.int32), np.empty((max(cap, 0), 2), np.float32), np.zeros(4, np.int32)
        offsets, runs, owner = np.zeros(max(cap, 0) + 1, np.int64), c_void_p(), c_void_p()
        check(self._api.visp_sam_generate_masks_rle_host(self._handle, p.ctypes.data, k.ctypes.data, n, *params, cap, int(min_mask_region_area), ii.ctypes.data,
                                                         fi.ctypes.data, counts.ctypes.data, offsets.ctypes.data, byref(runs), byref(owner)))
        self._sam_batch_n = n
        r = int(counts[0])
        return _rle_records(offsets, runs, owner, r, w, h), ii[:r], fi[:r], (r, *(int(c) for c in counts[1:]))

    def sam_generate_masks(self, points_per_side: int = 32, prompts=None, pred_iou_thresh=None, stability_thresh=None, stability_offset=None, nms_iou_thresh=None,
                           max_masks: int = 256, min_mask_region_area: int = 0, output_mode: str = "binary_mask"):
        """SAM's automatic mask generator on the last sam_encode (one crop layer, no crop-edge filter; min_mask_region_area as in SAM: holes and islands below
        that many pixels are removed and a second NMS runs, after which unchanged masks come first and changed ones behind them): the points_per_side^2 grid
        of sam_point_grid, or `prompts` (points and boxes as for sam_compute_batch). Thresholds default to SAM's (sam_generate_defaults). Returns at most
        max_masks records in order of predicted iou, each a dict with SAM's keys: segmentation (bool [h, w]), area, bbox [x, y, w, h] (of the mask, image
        pixels), predicted_iou, stability_score, and point_coords [[x, y]] for a point prompt or box [x0, y0, x1, y1] for a box prompt.
        output_mode "uncompressed_rle": segmentation is SAM's RLE dict {"size": [h, w], "counts": [...]}, encoded on the device (no mask byte is read back);
        every other key is as with "binary_mask"."""
        if output_mode not in ("binary_mask", "uncompressed_rle"):
            raise ValueError(f"unknown output_mode {output_mode!r}: one of 'binary_mask', 'uncompressed_rle'")
        raw = self.sam_generate_masks_raw if output_mode == "binary_mask" else self.sam_generate_masks_rle_raw
        return self._sam_generate_records(raw, output_mode == "binary_mask", points_per_side, prompts, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh,
                                          max_masks, min_mask_region_area)

    def sam_generate_masks_coco_rle(self, points_per_side: int = 32, prompts=None, pred_iou_thresh=None, stability_thresh=None, stability_offset=None, nms_iou_thresh=None,
                                    max_masks: int = 256, min_mask_region_area: int = 0):
        """sam_generate_masks in SAM's output mode coco_rle: segmentation is {"size": [h, w], "counts": bytes}, COCO's compressed counts string as pycocotools
        exchanges it, encoded and compressed on the device (visp_sam_generate_masks_coco_rle_host: neither a mask byte nor a run is read back); every other key
        is as with "uncompressed_rle"."""
        return self._sam_generate_records(self.sam_generate_masks_coco_rle_raw, False, points_per_side, prompts, pred_iou_thresh, stability_thresh, stability_offset,
                                          nms_iou_thresh, max_masks, min_mask_region_area)

    def sam_generate_masks_coco_rle_raw(self, prompts=None, points_per_side: int = 32, pred_iou_thresh=None, stability_thresh=None, stability_offset=None, nms_iou_thresh=None,
                                        max_masks: int = 256, min_mask_region_area: int = 0):
        """sam_generate_masks_rle_raw with the records' counts as compressed strings (bytes)"""
        p, k, params = self._sam_generate_args(prompts, points_per_side, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh)
        n, cap = len(k), int(max_masks)
        w, h = self.sam_image_extent() if n and cap > 0 else (0, 0)
        ii, fi, counts = np.empty((max(cap, 0), 8), np.int32), np.empty((max(cap, 0), 2), np.float32), np.zeros(4, np.int32)
        offsets, data, owner = np.zeros(max(cap, 0) + 1, np.int64), c_void_p(), c_void_p()
        check(self._api.visp_sam_generate_masks_coco_rle_host(self._handle, p.ctypes.data, k.ctypes.data, n, *params, cap, int(min_mask_region_area), ii.ctypes.data,
                                                              fi.ctypes.data, counts.ctypes.data, offsets.ctypes.data, byref(data), byref(owner)))
        self._sam_batch_n = n
        r = int(counts[0])
        return _string_records(offsets, data, owner, [[h, w]] * r), ii[:r], fi[:r], (r, *(int(c) for c in counts[1:]))

    def _sam_generate_records(self, raw, binary: bool, points_per_side, prompts, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, max_masks,
                              min_mask_region_area):
        """the records of sam_generate_masks from one of the raw calls"""
        p, k, _ = self._sam_generate_args(prompts, points_per_side, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh)
        masks, ii, fi, _ = raw([list(q[:c]) for q, c in zip(p, k)], points_per_side, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh, max_masks,
                               min_mask_region_area)
        out = []
        for m, row, (piou, stab) in zip(masks, ii, fi):
            prompt = int(row[0])
            rec = dict(segmentation=m == 255 if binary else m, area=int(row[6]), bbox=[int(v) for v in row[2:6]], predicted_iou=float(piou), stability_score=float(stab))
            if k[prompt] == 2:
                rec["point_coords"] = [[int(p[prompt, 0]), int(p[prompt, 1])]]
            else:
                rec["box"] = [int(v) for v in p[prompt]]
            out.append(rec)
        return out

    def sam_generate_masks_device(self, prompts, masks_dev: int, info_i32_dev: int, info_f32_dev: int, counts_dev: int, max_masks: int = 256, pred_iou_thresh=None,
                                  stability_thresh=None, stability_offset=None, nms_iou_thresh=None, stream: int | None = None, min_mask_region_area: int = 0):
        """The same into device buffers (addresses): masks u8 [max_masks, h, w], info i32 [max_masks, 8], info f32 [max_masks, 2], counts i32 [2]; rows and masks
        at and behind counts[0] stay untouched. Nothing waits for the device when a stream is given. min_mask_region_area > 0: counts i32 [4] and SAM's order
        behind the cleaning, as sam_generate_masks_raw describes."""
        p, k, params = self._sam_generate_args(prompts, 32, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh)
        if int(min_mask_region_area):
            check(self._api.visp_sam_generate_masks_clean_device(self._handle, p.ctypes.data, k.ctypes.data, len(k), *params, int(max_masks), int(min_mask_region_area),
                                                                 masks_dev, info_i32_dev, info_f32_dev, counts_dev, stream))
        else:
            check(self._api.visp_sam_generate_masks_device(self._handle, p.ctypes.data, k.ctypes.data, len(k), *params, int(max_masks), masks_dev, info_i32_dev,
                                                           info_f32_dev, counts_dev, stream))
        self._sam_batch_n = len(k)

    def sam_generate_last_split(self) -> dict:
        """ms of the last generate call by HIP events, recorded while timing is enabled (enable_timing): decode, scoring, rank + NMS, output masks."""
        out = (ctypes.c_float * 4)()
        check(self._api.visp_sam_generate_last_split(self._handle, out))
        return dict(zip(("decode_ms", "scoring_ms", "rank_nms_ms", "output_ms"), (float(v) for v in out)))

    def sam_generate_last_split5(self) -> dict:
        """sam_generate_last_split with the cleaning stage of the last call as a fifth figure, and that stage's parts: clean, records + second NMS, gather."""
        out, parts = (ctypes.c_float * 5)(), (ctypes.c_float * 3)()
        check(self._api.visp_sam_generate_last_split5(self._handle, out))
        check(self._api.visp_sam_generate_last_clean_split(self._handle, parts))
        names = ("decode_ms", "scoring_ms", "rank_nms_ms", "output_ms", "cleaning_ms", "clean_ms", "records_nms2_ms", "gather_ms")
        return dict(zip(names, (float(v) for v in (*out, *parts))))

    def sam_encode_batch(self, images: np.ndarray) -> np.ndarray:
        """images: uint8 [B, 1024, 1024, 3] on the host -> image embeddings float32 [B, 64, 64, 256]."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert (h, w, c) == (1024, 1024, 3)
        out = np.empty((b, 64, 64, 256), np.float32)
        check(self._api.visp_sam_encode_batch_host(self._handle, imgs.ctypes.data, b, out.ctypes.data))
        return out

    def sam_encode_batch_device(self, rgb_dev: int, batch: int, out_dev: int, stream: int | None = None):
        check(self._api.visp_sam_encode_batch_device(self._handle, rgb_dev, batch, out_dev, stream))


def sam_point_grid(n_per_side: int, w: int, h: int) -> np.ndarray:
    """The point prompts of a "segment everything" pass: pixel centres of an n x n grid over a w x h image, int32 [n * n, 2] of (x, y), row by row."""
    xs = ((np.arange(n_per_side) + 0.5) * w / n_per_side).astype(np.int32)
    ys = ((np.arange(n_per_side) + 0.5) * h / n_per_side).astype(np.int32)
    gx, gy = np.meshgrid(xs, ys)
    return np.stack([gx.reshape(-1), gy.reshape(-1)], axis=1).astype(np.int32)


def sam_generate_defaults() -> dict:
    """SAM's automatic mask generator defaults, as the library holds them (visp_sam_generate_defaults)."""
    out = (ctypes.c_float * 4)()
    check(lib.get_lib().visp_sam_generate_defaults(out))
    return dict(zip(("pred_iou_thresh", "stability_thresh", "stability_offset", "nms_iou_thresh"), (float(v) for v in out)))


class DepthPipeline:
    """Overlapped host pipeline over visp_depthany_pipeline_* (include/visp_c_api.h): submit() returns a ticket at once, wait()
    returns that batch's [batch, h, w] f32 depth maps; up to n_slots - 1 batches may be in flight."""

    def __init__(self, model: "Model", batch: int, w: int, h: int, n_slots: int = 3):
        self._api, self._model = model._api, model
        self.batch, self.w, self.h, self.n_slots = batch, w, h, n_slots
        p = c_void_p()
        check(self._api.visp_depthany_pipeline_create(model._handle, batch, w, h, n_slots, byref(p)))
        self._p = p

    def input_view(self) -> np.ndarray:
        """The next slot's pinned input buffer as a writable [batch, h, w, 3] uint8 array (fill it, then submit(None))."""
        ptr = c_void_p()
        check(self._api.visp_depthany_pipeline_input(self._p, byref(ptr)))
        n = self.batch * self.h * self.w * 3
        return np.frombuffer((ctypes.c_uint8 * n).from_address(ptr.value), np.uint8).reshape(self.batch, self.h, self.w, 3)

    def submit(self, images: np.ndarray | None) -> int:
        t = ctypes.c_int32()
        if images is not None:
            images = np.ascontiguousarray(images, dtype=np.uint8)
            assert images.shape == (self.batch, self.h, self.w, 3)
        check(self._api.visp_depthany_pipeline_submit(self._p, images.ctypes.data if images is not None else None, byref(t)))
        return t.value

    def wait(self, ticket: int, copy: bool = True) -> np.ndarray:
        ptr = c_void_p()
        check(self._api.visp_depthany_pipeline_wait(self._p, ticket, byref(ptr)))
        n = self.batch * self.h * self.w
        a = np.frombuffer((ctypes.c_float * n).from_address(ptr.value), np.float32).reshape(self.batch, self.h, self.w)
        return a.copy() if copy else a

    def close(self):
        if getattr(self, "_p", None):
            self._api.visp_depthany_pipeline_destroy(self._p)
            self._p = None

    def __del__(self):
        self.close()


def image_scale(image: np.ndarray, width: int, height: int, format: ImageFormat = ImageFormat.rgb_u8, device: "Device | None" = None) -> np.ndarray:
    """The reference's image_scale (src/visp/image.cpp:328-356): [h, w, ch] u8 or f32 -> [height, width, ch]. On the host by default; with a
    device, on that device (up, one fused launch, down), where a leading batch axis [B, h, w, ch] is allowed too. The same bytes either way."""
    api = lib.get_lib()
    is_f32 = format.value >= ImageFormat.rgba_f32.value
    img = np.ascontiguousarray(image, dtype=np.float32 if is_f32 else np.uint8)
    ch = _CHANNELS[format.value]
    if device is not None:
        batched = img.ndim == (3 if ch == 1 else 4)
        b, (h, w) = (img.shape[0] if batched else 1), img.shape[1:3] if batched else img.shape[:2]
        out = np.empty(((b,) if batched else ()) + (height, width) + (() if ch == 1 else (ch,)), img.dtype)
        check(api.visp_image_scale_batch_host(device._handle, img.ctypes.data, format.value, b, w, h, out.ctypes.data, width, height))
        return out
    h, w = img.shape[:2]
    view = lib.ImageView(w, h, w * ch * img.itemsize, format.value, img.ctypes.data)
    out_view, out_data = lib.ImageView(), c_void_p()
    check(api.visp_image_scale(byref(view), width, height, byref(out_view), byref(out_data)))
    try:
        n = out_view.height * out_view.stride
        buf = (ctypes.c_uint8 * n).from_address(out_view.data)
        res = np.frombuffer(buf, img.dtype).reshape(out_view.height, out_view.width, ch).copy()
    finally:
        api.visp_image_destroy(out_data)
    return res[..., 0] if ch == 1 else res


def image_scale_batch_device(src_dev: int, format: ImageFormat, batch: int, w: int, h: int, dst_dev: int, out_w: int, out_h: int,
                             device: "Device | None" = None, stream: int | None = None):
    """image_scale on device-resident batches (addresses): src [batch, h, w, ch] -> dst [batch, out_h, out_w, ch] of one format, one fused launch,
    the bytes of image_scale. Returns with the stream synchronised (the tap tables live for the call)."""
    check(lib.get_lib().visp_image_scale_batch_device(device._handle if device is not None else None, src_dev, format.value, int(batch), int(w), int(h), dst_dev,
                                                      int(out_w), int(out_h), stream))


# ---- the matting image ops (reference include/visp/image.h:141-170). Arrays are [h, w] or [h, w, ch]; a view of a wider array keeps its row stride.
def _view_of(image: np.ndarray, format: ImageFormat):
    """(ImageView, the array that owns its memory): uint8 or float32 by the format, rows may be strided, pixels are contiguous."""
    dtype = np.float32 if format.value >= ImageFormat.rgba_f32.value else np.uint8
    img = np.asarray(image, dtype=dtype)
    ch = _CHANNELS[format.value]
    if img.ndim == 2:
        img = img[..., None]
    if img.ndim != 3 or img.shape[2] != ch:
        raise ValueError(f"expected an array of {ch} channel(s) for {format.name}, got shape {image.shape}")
    if img.strides[2] != img.itemsize or img.strides[1] != ch * img.itemsize or img.strides[0] < img.shape[1] * ch * img.itemsize:
        img = np.ascontiguousarray(img)
    return lib.ImageView(img.shape[1], img.shape[0], img.strides[0], format.value, img.ctypes.data), img


def _take(out_view, out_data) -> np.ndarray:
    api = lib.get_lib()
    try:
        fmt = out_view.format
        dtype, ch = (np.float32 if fmt >= ImageFormat.rgba_f32.value else np.uint8), _CHANNELS[fmt]
        buf = (ctypes.c_uint8 * (out_view.height * out_view.stride)).from_address(out_view.data)
        res = np.frombuffer(buf, dtype).reshape(out_view.height, out_view.width, ch).copy()
    finally:
        api.visp_image_destroy(out_data)
    return res[..., 0] if ch == 1 else res


def _image_op(name: str, views: list, *args, on: tuple = ()) -> np.ndarray:
    """Calls the C entry `name`(*on, views..., *args, out_view, out_data) and takes the library-owned result; views: what _view_of returns."""
    out_view, out_data = lib.ImageView(), c_void_p()
    check(getattr(lib.get_lib(), name)(*on, *(byref(v) for v, _ in views), *args, byref(out_view), byref(out_data)))
    return _take(out_view, out_data)


def _on(device: "Device | None") -> tuple:
    return (device._handle if device is not None else None,)  # NULL: the calling thread's current HIP device


def image_blur(image: np.ndarray, radius: int, device: Device | None = None) -> np.ndarray:
    """Box filter of size 2 radius + 1 with replicated edges: f32 [h, w] (alpha_f32) or [h, w, 4] (rgba_f32). device None: the current HIP device."""
    fmt = ImageFormat.alpha_f32 if np.ndim(image) == 2 else ImageFormat.rgba_f32
    return _image_op("visp_image_blur", [_view_of(image, fmt)], int(radius), on=_on(device))


def image_erosion(mask: np.ndarray, radius: int, device: Device | None = None) -> np.ndarray:
    """Minimum over the (2 radius + 1)^2 neighbourhood: [h, w] uint8 (alpha_u8) or float32 (alpha_f32), same type out."""
    fmt = ImageFormat.alpha_u8 if np.asarray(mask).dtype == np.uint8 else ImageFormat.alpha_f32
    return _image_op("visp_image_erosion", [_view_of(mask, fmt)], int(radius), on=_on(device))


REGION_MODES = {"holes": 1, "islands": 2, "both": 3}


def remove_small_regions(masks: np.ndarray, min_area: int, mode: str = "both", device: Device | None = None):
    """SAM's remove_small_regions on the device: masks uint8 [n, h, w] or [h, w] (non-zero = foreground) -> (masks, changed). "holes": background components
    of fewer than min_area pixels (8-connectivity, none exempt for touching the border) become 255; "islands": such foreground components become 0, but where
    every one is small the largest stays; "both": the holes, then the islands of the result. Only flipped pixels differ from the input. changed: bool [n], or
    a bool for a single mask."""
    if mode not in REGION_MODES:
        raise ValueError(f"unknown mode {mode!r}: one of {sorted(REGION_MODES)}")
    m = np.array(masks, dtype=np.uint8, order="C", copy=True)
    if m.ndim not in (2, 3):
        raise ValueError(f"expected masks [n, h, w] or [h, w], got shape {m.shape}")
    n, (h, w) = (1 if m.ndim == 2 else m.shape[0]), m.shape[-2:]
    changed = np.zeros(max(n, 1), np.int32)
    check(lib.get_lib().visp_image_remove_small_regions_host(m.ctypes.data, n, w, h, int(min_area), REGION_MODES[mode], changed.ctypes.data, *_on(device)))
    return m, (bool(changed[0]) if m.ndim == 2 else changed[:n].astype(bool))


def remove_small_regions_device(masks_dev: int, n: int, w: int, h: int, min_area: int, mode: str = "both", changed_dev: int | None = None, device: Device | None = None,
                                stream: int | None = None):
    """The same in place on device-resident masks u8 [n, h, w] (addresses; changed i32 [n] optional). Returns with the work done."""
    if mode not in REGION_MODES:
        raise ValueError(f"unknown mode {mode!r}: one of {sorted(REGION_MODES)}")
    check(lib.get_lib().visp_image_remove_small_regions_device(masks_dev, int(n), int(w), int(h), int(min_area), REGION_MODES[mode], changed_dev, stream, *_on(device)))


def _rle_records(offsets, runs_ptr, owner, count: int, w: int, h: int) -> list:
    """the library-owned runs of an RLE host call as SAM's dicts, one per mask; releases the buffer"""
    try:
        total = int(offsets[count])
        runs = np.ctypeslib.as_array(ctypes.cast(runs_ptr, ctypes.POINTER(ctypes.c_uint32)), (total,)).copy() if total else np.empty(0, np.uint32)
    finally:
        lib.get_lib().visp_rle_destroy(owner)
    return [{"size": [int(h), int(w)], "counts": runs[int(offsets[b]):int(offsets[b + 1])].tolist()} for b in range(count)]


def mask_to_rle(masks: np.ndarray, device: Device | None = None):
    """COCO's uncompressed RLE on the device, SAM's mask_to_rle_pytorch: masks [n, h, w] or [h, w] (non-zero = foreground) -> a list of
    {"size": [h, w], "counts": [...]} (one dict for a single mask). Pixels are visited column by column; counts alternate from background, the first is 0 when
    the top-left pixel is foreground."""
    a = np.asarray(masks)
    m = np.ascontiguousarray(a if a.dtype == np.uint8 else a != 0, dtype=np.uint8)
    if m.ndim not in (2, 3):
        raise ValueError(f"expected masks [n, h, w] or [h, w], got shape {m.shape}")
    n, (h, w) = (1 if m.ndim == 2 else m.shape[0]), m.shape[-2:]
    offsets, runs, owner = np.zeros(max(n, 0) + 1, np.int64), c_void_p(), c_void_p()
    check(lib.get_lib().visp_image_rle_encode_host(m.ctypes.data, n, w, h, offsets.ctypes.data, byref(runs), byref(owner), *_on(device)))
    out = _rle_records(offsets, runs, owner, n, w, h)
    return out[0] if m.ndim == 2 else out


def mask_to_rle_device(masks_dev: int, n: int, w: int, h: int, runs_dev: int | None, run_stride: int, n_runs_dev: int, counts_dev: int | None = None,
                       device: Device | None = None, stream: int | None = None):
    """The same on device-resident masks u8 [n, h, w] (addresses): n_runs i32 [n] receives each mask's true number of runs, runs u32 [n, run_stride] the first
    min(n_runs, run_stride) of them (runs_dev None or run_stride 0: the counts alone). counts_dev: a device i32, masks at and behind counts[0] are skipped.
    Returns with the work done."""
    check(lib.get_lib().visp_image_rle_encode_device(masks_dev, int(n), int(w), int(h), counts_dev, runs_dev, int(run_stride), n_runs_dev, stream, *_on(device)))


def rle_to_mask(rle: dict) -> np.ndarray:
    """SAM's rle_to_mask on the host: {"size": [h, w], "counts": [...]} -> bool [h, w]."""
    h, w = rle["size"]
    flat = np.zeros(h * w, bool)
    pos, value = 0, False
    for c in rle["counts"]:
        flat[pos:pos + c] = value
        pos += c
        value = not value
    return flat.reshape(w, h).T


def _rle_rows(rles, device: Device | None = None) -> tuple:
    """RLE dicts of one extent -> (offsets i64 [n + 1], runs u32, w, h): the CSR rows of the C entries. Records whose counts are a compressed string (bytes or
    str) are decompressed on the device first."""
    if not rles:
        raise ValueError("expected at least one RLE record")
    h, w = (int(v) for v in rles[0]["size"])
    if any([int(v) for v in r["size"]] != [h, w] for r in rles):
        raise ValueError(f"the records differ in size: expected [{h}, {w}] in all of them")
    packed = [i for i, r in enumerate(rles) if isinstance(r["counts"], (bytes, str))]
    if packed:
        rles = list(rles)
        for i, r in zip(packed, rle_decompress([rles[i] for i in packed], device)):
            rles[i] = r
    return *_run_rows(rles), w, h


def _run_rows(rles) -> tuple:
    """the list counts of RLE dicts -> (offsets i64 [n + 1], runs u32), one row behind the other"""
    rows = [np.asarray(r["counts"], np.int64) for r in rles]
    if any(c.size and (c.min() < 0 or c.max() >= 2 ** 32) for c in rows):
        raise ValueError("counts must lie in 0 .. 2^32 - 1")
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([c.size for c in rows], out=offsets[1:])
    runs = np.concatenate(rows).astype(np.uint32) if offsets[-1] else np.zeros(1, np.uint32)
    return offsets, runs


def _string_records(byte_offsets, data_ptr, owner, sizes) -> list:
    """the library-owned strings of a compress call as records {"size": .., "counts": bytes}, one per entry of sizes; releases the buffer"""
    try:
        data = ctypes.string_at(data_ptr, int(byte_offsets[len(sizes)])) if len(sizes) and byte_offsets[len(sizes)] else b""
    finally:
        lib.get_lib().visp_rle_destroy(owner)
    return [{"size": [int(v) for v in s], "counts": data[int(byte_offsets[b]):int(byte_offsets[b + 1])]} for b, s in enumerate(sizes)]


def rle_compress(rles, device: Device | None = None):
    """pycocotools' compressed form on the device (its rleToString): records {"size": [h, w], "counts": [...]} -> the same records with counts as bytes, the
    string a COCO file holds in segmentation.counts (.decode("ascii") for json). A list in, a list out; one dict in, one dict out. Counts lie below 2^31."""
    single = isinstance(rles, dict)
    recs = [rles] if single else list(rles)
    if not recs:
        raise ValueError("expected at least one RLE record")
    offsets, runs = _run_rows(recs)
    byte_offsets, data, owner = np.zeros(len(recs) + 1, np.int64), c_void_p(), c_void_p()
    check(lib.get_lib().visp_image_rle_compress_host(offsets.ctypes.data, runs.ctypes.data, len(recs), byte_offsets.ctypes.data, byref(data), byref(owner), *_on(device)))
    out = _string_records(byte_offsets, data, owner, [r["size"] for r in recs])
    return out[0] if single else out


def rle_decompress(rles, device: Device | None = None):
    """The way back (pycocotools' rleFrString): records whose counts are bytes, or str read as ASCII -> records with list counts. A malformed string is refused;
    the message names the record, the byte and the status (1 a byte outside 48 .. 111, 2 unterminated, 3 a value of more than 7 bytes, 4 a count outside
    0 .. 2^31 - 1)."""
    single = isinstance(rles, dict)
    recs = [rles] if single else list(rles)
    if not recs:
        raise ValueError("expected at least one RLE record")
    rows = [r["counts"].encode("ascii") if isinstance(r["counts"], str) else bytes(r["counts"]) for r in recs]
    byte_offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(c) for c in rows], out=byte_offsets[1:])
    data = np.frombuffer(b"".join(rows) or b"\0", np.uint8)
    offsets, runs, owner = np.zeros(len(rows) + 1, np.int64), c_void_p(), c_void_p()
    check(lib.get_lib().visp_image_rle_decompress_host(byte_offsets.ctypes.data, data.ctypes.data, len(rows), offsets.ctypes.data, byref(runs), byref(owner), *_on(device)))
    try:
        total = int(offsets[-1])
        flat = np.ctypeslib.as_array(ctypes.cast(runs, ctypes.POINTER(ctypes.c_uint32)), (total,)).copy() if total else np.empty(0, np.uint32)
    finally:
        lib.get_lib().visp_rle_destroy(owner)
    out = [{"size": [int(v) for v in r["size"]], "counts": flat[int(offsets[b]):int(offsets[b + 1])].tolist()} for b, r in enumerate(recs)]
    return out[0] if single else out


def mask_to_coco_rle(masks: np.ndarray, device: Device | None = None):
    """mask_to_rle and rle_compress in one call on the device (pycocotools' encode): masks [n, h, w] or [h, w] -> records with counts as bytes. The runs never
    leave the device."""
    a = np.asarray(masks)
    m = np.ascontiguousarray(a if a.dtype == np.uint8 else a != 0, dtype=np.uint8)
    if m.ndim not in (2, 3):
        raise ValueError(f"expected masks [n, h, w] or [h, w], got shape {m.shape}")
    n, (h, w) = (1 if m.ndim == 2 else m.shape[0]), m.shape[-2:]
    byte_offsets, data, owner = np.zeros(max(n, 0) + 1, np.int64), c_void_p(), c_void_p()
    check(lib.get_lib().visp_image_rle_encode_compressed_host(m.ctypes.data, n, w, h, byte_offsets.ctypes.data, byref(data), byref(owner), *_on(device)))
    out = _string_records(byte_offsets, data, owner, [[h, w]] * n)
    return out[0] if m.ndim == 2 else out


def rle_decode(rles, value: int = 1, device: Device | None = None) -> np.ndarray:
    """pycocotools' decode on the device: the record dicts mask_to_rle and sam_generate_masks return ({"size": [h, w], "counts": [...]}, all of one size) ->
    uint8 [n, h, w] with foreground bytes `value` ([h, w] for a single dict). A record whose counts do not sum to h * w is refused."""
    single = isinstance(rles, dict)
    offsets, runs, w, h = _rle_rows([rles] if single else list(rles), device)
    out = np.empty((len(offsets) - 1, h, w), np.uint8)
    check(lib.get_lib().visp_image_rle_decode_host(offsets.ctypes.data, runs.ctypes.data, len(offsets) - 1, w, h, int(value), out.ctypes.data, *_on(device)))
    return out[0] if single else out


def rle_decode_device(runs_dev: int, offsets_dev: int, n: int, w: int, h: int, masks_dev: int, value: int = 1, counts_dev: int | None = None, status_dev: int | None = None,
                      area_dev: int | None = None, device: Device | None = None, stream: int | None = None):
    """The same on device-resident rows (addresses): runs u32 and offsets i64 [n + 1] as the encoder's packed form -> masks u8 [n, h, w]; status i32 [n]
    (0 exact, 1 short, 2 long) and area i64 [n] optional. counts_dev: a device i32, masks at and behind counts[0] are skipped. Returns with the work done."""
    check(lib.get_lib().visp_image_rle_decode_device(runs_dev, offsets_dev, int(n), int(w), int(h), counts_dev, int(value), masks_dev, status_dev, area_dev, stream,
                                                     *_on(device)))


def rle_area(rles) -> np.ndarray:
    """pycocotools' area: the foreground pixels of each record, int64 [n] (a scalar for a single dict). Host code."""
    single = isinstance(rles, dict)
    offsets, runs, _, _ = _rle_rows([rles] if single else list(rles))
    area = np.zeros(len(offsets) - 1, np.int64)
    check(lib.get_lib().visp_image_rle_area_host(offsets.ctypes.data, runs.ctypes.data, len(area), area.ctypes.data))
    return int(area[0]) if single else area


def mask_iou(a, b, iscrowd=None, device: Device | None = None, return_intersection: bool = False):
    """pycocotools' iou on the device: a and b are each a list of record dicts or masks [n, h, w] (non-zero = foreground), all of one extent -> float32 [na, nb] =
    intersection / union, or intersection / area of a where iscrowd[j] is set; 0 where that denominator is 0. return_intersection: also int32 [na, nb]."""
    keep, sides = [], []
    for s in (a, b):
        if isinstance(s, np.ndarray):
            m = np.ascontiguousarray(s if s.dtype == np.uint8 else s != 0, dtype=np.uint8)
            if m.ndim != 3:
                raise ValueError(f"expected masks [n, h, w], got shape {m.shape}")
            keep.append(m)
            sides.append((m.ctypes.data, None, None, m.shape[0], m.shape[2], m.shape[1]))
        else:
            offsets, runs, w, h = _rle_rows(list(s), device)
            keep += [offsets, runs]
            sides.append((None, runs.ctypes.data, offsets.ctypes.data, len(offsets) - 1, w, h))
    na, nb = sides[0][3], sides[1][3]
    crowd = None if iscrowd is None else np.ascontiguousarray(np.asarray(iscrowd) != 0, dtype=np.uint8)
    if crowd is not None and crowd.shape != (nb,):
        raise ValueError(f"iscrowd: expected {nb} flags, got shape {crowd.shape}")
    iou, inter = np.empty((na, nb), np.float32), np.empty((na, nb), np.int32)
    check(lib.get_lib().visp_image_mask_iou_host(*sides[0], *sides[1], None if crowd is None else crowd.ctypes.data, iou.ctypes.data, inter.ctypes.data, *_on(device)))
    return (iou, inter) if return_intersection else iou


def mask_iou_device(a: tuple, b: tuple, iou_dev: int, iscrowd_dev: int | None = None, inter_dev: int | None = None, device: Device | None = None, stream: int | None = None):
    """The same on device-resident sides (addresses): each of a, b is (masks_dev, None, None, n, w, h) or (None, runs_dev, offsets_dev, n, w, h); iou f32 [na, nb],
    inter i32 [na, nb] optional, iscrowd u8 [nb] optional. Returns with the work done."""
    check(lib.get_lib().visp_image_mask_iou_device(*a, *b, iscrowd_dev, iou_dev, inter_dev, stream, *_on(device)))


def _polygon_rows(polygons) -> tuple:
    """polygons, each [k, 2] or COCO's flat [x0, y0, x1, y1, ..] -> (xy f64 [total, 2], poly_offsets i64 [n + 1])"""
    rows = [np.asarray(p, np.float64).reshape(-1, 2) for p in polygons]
    if not rows:
        raise ValueError("expected at least one polygon")
    offsets = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offsets[1:])
    return np.ascontiguousarray(np.concatenate(rows + [np.zeros((1, 2))])), offsets  # an address also without vertices


def poly_to_rle(polygons, h: int, w: int, device: Device | None = None) -> list:
    """pycocotools' frPoly on the device: polygons (each [k, 2], or COCO's flat [x0, y0, x1, y1, ..]) on an h x w image -> one record
    {"size": [h, w], "counts": [...]} per polygon. A NaN, a coordinate beyond 2^20 or a polygon without vertices is refused; the message names the polygon."""
    xy, poff = _polygon_rows(polygons)
    offsets, runs, owner = np.zeros(len(poff), np.int64), c_void_p(), c_void_p()
    check(lib.get_lib().visp_image_rle_from_poly_host(xy.ctypes.data, poff.ctypes.data, len(poff) - 1, int(w), int(h), offsets.ctypes.data, byref(runs), byref(owner), *_on(device)))
    return _rle_records(offsets, runs, owner, len(poff) - 1, w, h)


def bbox_to_rle(boxes, h: int, w: int, device: Device | None = None) -> list:
    """pycocotools' frBbox: boxes [n, 4] = (x, y, bw, bh) -> one record per box, each box as its four-vertex polygon through poly_to_rle's kernels."""
    b = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4))
    offsets, runs, owner = np.zeros(len(b) + 1, np.int64), c_void_p(), c_void_p()
    check(lib.get_lib().visp_image_rle_from_bbox_host(b.ctypes.data, len(b), int(w), int(h), offsets.ctypes.data, byref(runs), byref(owner), *_on(device)))
    return _rle_records(offsets, runs, owner, len(b), w, h)


def rle_merge(records, intersect: bool = False, device: Device | None = None):
    """pycocotools' merge on the device: a list of records -> the record of their union (of their intersection with intersect); a list of lists of records ->
    one merged record per inner list, an empty inner list giving an empty mask. All records have one size."""
    recs = list(records)
    single = not recs or isinstance(recs[0], dict)
    groups = [recs] if single else [list(g) for g in recs]
    flat = [r for g in groups for r in g]
    offsets, runs, w, h = _rle_rows(flat, device)
    goff = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(g) for g in groups], out=goff[1:])
    out_offsets, out_runs, owner = np.zeros(len(groups) + 1, np.int64), c_void_p(), c_void_p()
    check(lib.get_lib().visp_image_rle_merge_host(offsets.ctypes.data, runs.ctypes.data, len(flat), goff.ctypes.data, len(groups), w, h, int(bool(intersect)),
                                                  out_offsets.ctypes.data, byref(out_runs), byref(owner), *_on(device)))
    out = _rle_records(out_offsets, out_runs, owner, len(groups), w, h)
    return out[0] if single else out


def rle_to_bbox(rles, device: Device | None = None) -> np.ndarray:
    """pycocotools' toBbox on the device: records -> int32 [n, 4] = (x, y, bw, bh), the tight box of each record's foreground, zeros for an empty mask
    ([4] for a single dict)."""
    single = isinstance(rles, dict)
    offsets, runs, w, h = _rle_rows([rles] if single else list(rles), device)
    boxes = np.zeros((len(offsets) - 1, 4), np.int32)
    check(lib.get_lib().visp_image_rle_to_bbox_host(offsets.ctypes.data, runs.ctypes.data, len(boxes), w, h, boxes.ctypes.data, *_on(device)))
    return boxes[0] if single else boxes


def fr_py_objects(obj, h: int, w: int, device: Device | None = None):
    """pycocotools' frPyObjects: an RLE dict is passed through as it is; a list of boxes ([n, 4] array, or lists of four numbers) gives a list of box records;
    a list of polygon lists (each object a list of flat [x0, y0, x1, y1, ..] polygons of six numbers or more) gives one merged record per object."""
    if isinstance(obj, dict):
        return obj
    if isinstance(obj, np.ndarray) and obj.ndim == 2 and obj.shape[1] == 4:
        return bbox_to_rle(obj, h, w, device)
    objs = list(obj)
    if not objs:
        raise ValueError("expected at least one object")
    flat = [len(o) > 0 and np.isscalar(o[0]) for o in objs]  # numbers, not polygons
    if all(flat) and all(len(o) == 4 for o in objs):
        return bbox_to_rle(objs, h, w, device)
    if all(flat):  # one object given as its polygons' coordinates
        return rle_merge(poly_to_rle(objs, h, w, device), device=device)
    records, at, out = poly_to_rle([p for o in objs for p in o], h, w, device), 0, []
    for o in objs:
        out.append(records[at:at + len(o)])
        at += len(o)
    return rle_merge(out, device=device)


def image_estimate_foreground(image: np.ndarray, mask: np.ndarray, radius: int = 30, device: Device | None = None) -> np.ndarray:
    """image f32 [h, w, 4] (rgba_f32), mask f32 [h, w] -> f32 [h, w, 4]: foreground colours, alpha = mask (blur-fusion, two stages)."""
    return _image_op("visp_image_estimate_foreground", [_view_of(image, ImageFormat.rgba_f32), _view_of(mask, ImageFormat.alpha_f32)], int(radius), on=_on(device))


def image_alpha_composite(fg: np.ndarray, bg: np.ndarray, mask: np.ndarray, device: Device | None = None) -> np.ndarray:
    """fg uint8 [h, w, 4], bg uint8 [h, w, 3 or 4], mask uint8 [h, w] -> uint8 [h, w, 4] = fg * alpha + bg * (1 - alpha), alpha 255."""
    bg_fmt = ImageFormat.rgb_u8 if np.shape(bg)[-1] == 3 else ImageFormat.rgba_u8
    return _image_op("visp_image_alpha_composite", [_view_of(fg, ImageFormat.rgba_u8), _view_of(bg, bg_fmt), _view_of(mask, ImageFormat.alpha_u8)], on=_on(device))


def image_set_alpha(image: np.ndarray, alpha: np.ndarray, format: ImageFormat = ImageFormat.rgba_u8) -> np.ndarray:
    """A copy of image (uint8 [h, w, 4] in `format`: rgba / bgra / argb) with its alpha channel set from alpha (uint8 [h, w]). Host code."""
    return _image_op("visp_image_set_alpha", [_view_of(image, format), _view_of(alpha, ImageFormat.alpha_u8)])


def image_to_mask(image: np.ndarray, format: ImageFormat = ImageFormat.rgba_u8) -> np.ndarray:
    """The first channel of a uint8 image as a mask uint8 [h, w]. Host code."""
    return _image_op("visp_image_to_mask", [_view_of(image, format)])


def estimate_foreground_batch_device(img_dev: int, img_format: ImageFormat, mask_dev: int, batch: int, w: int, h: int, out_dev: int,
                                     out_format: ImageFormat = ImageFormat.rgba_u8, radius: int = 30, device: Device | None = None, stream: int | None = None):
    """The estimator on device-resident batches: img [batch, h, w] pixels of rgba_f32 / rgb_u8 / rgba_u8, mask f32 [batch, h, w] -> out [batch, h, w, 4]."""
    check(lib.get_lib().visp_image_estimate_foreground_batch_device(device._handle if device is not None else None, img_dev, img_format.value, mask_dev, batch, w, h,
                                                                    int(radius), out_dev, out_format.value, stream))


def esrgan_tile_layout(w: int, h: int, scale: int = 1) -> dict:
    v = (c_int32 * 8)()
    check(get_lib().visp_esrgan_tile_layout(w, h, scale, v))
    return dict(zip(("image_w", "image_h", "overlap_x", "overlap_y", "n_x", "n_y", "tile_w", "tile_h"), [int(x) for x in v]))


class DeviceBuffer:
    """Raw device allocation through the vx_* runtime ABI (tests and bench use it so the hot path
    never depends on torch tensors)."""

    def __init__(self, nbytes: int):
        self._api = get_lib()
        self.nbytes = nbytes
        p = c_void_p()
        vx_check(self._api.vx_malloc(byref(p), nbytes))
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a: np.ndarray):
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        vx_check(b._api.vx_memcpy_h2d(b.ptr, a.ctypes.data, a.nbytes, None))
        vx_check(b._api.vx_stream_sync(None))
        return b

    def to_numpy(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        vx_check(self._api.vx_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, None))
        return out

    def zero(self):
        vx_check(self._api.vx_memset(self.ptr, 0, self.nbytes, None))
        vx_check(self._api.vx_stream_sync(None))

    def __del__(self):
        if getattr(self, "ptr", None):
            self._api.vx_free(self.ptr)
            self.ptr = None


class SwinEncoder(Model):
    """The SWIN encoder of a birefnet GGUF on its own (reference swin_encode, src/visp/arch/swin.cpp:237-262, behind
    birefnet::encode); the whole BiRefNet (encoder + decoder) is Model.load(..., Arch.birefnet). Outputs are the four normed
    stage maps, f32 [B, h_i, w_i, C_i]."""

    @classmethod
    def load(cls, path, device: Device):
        api = get_lib()
        handle = c_void_p()
        check(api.visp_swin_load(lib.path_to_char_p(path), device._handle, byref(handle)))
        return cls(api, handle, Arch.birefnet, device)

    def output_dims(self, w: int, h: int):
        d = (c_int32 * 12)()
        check(self._api.visp_swin_output_dims(self._handle, w, h, d))
        return [(d[3 * i], d[3 * i + 1], d[3 * i + 2]) for i in range(4)]  # (w_i, h_i, C_i)

    def encode_batch(self, images: np.ndarray):
        """images: uint8 [B, h, w, 3] on the host -> list of four f32 arrays [B, h_i, w_i, C_i]."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert c == 3
        outs = [np.empty((b, hh, ww, cc), np.float32) for ww, hh, cc in self.output_dims(w, h)]
        ptrs = (c_void_p * 4)(*[o.ctypes.data for o in outs])
        check(self._api.visp_swin_encode_batch_host(self._handle, imgs.ctypes.data, b, w, h, ptrs))
        return outs

    def encode_batch_device(self, rgb_dev: int, batch: int, w: int, h: int, outs_dev, stream: int | None = None):
        check(self._api.visp_swin_encode_batch_device(self._handle, rgb_dev, batch, w, h, (c_void_p * 4)(*outs_dev), stream))


class Migan(Model):
    """MI-GAN inpainting (reference migan_load_model / migan_compute, vision.h:257-279). Loaded through visp_migan_load:
    visp_model_load keeps refusing the family."""

    @classmethod
    def load(cls, path, device: Device):
        api = get_lib()
        handle = c_void_p()
        check(api.visp_migan_load(lib.path_to_char_p(path), device._handle, byref(handle)))
        return cls(api, handle, Arch.migan, device)

    @property
    def info(self) -> dict:
        i = lib.MiganInfo()
        check(self._api.visp_migan_get_info(self._handle, byref(i)))
        return dict(resolution=i.resolution, channels=[i.channels[k] for k in range(i.n_levels)])

    def compute(self, image: np.ndarray, mask: np.ndarray, format: ImageFormat | None = None) -> np.ndarray:
        """image u8 [h, w, 3 | 4], mask u8 [h, w] (alpha_u8) of any extent -> rgba u8 [h, w, 4], alpha = mask."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        msk = np.ascontiguousarray(mask, dtype=np.uint8)
        h, w, c = img.shape
        fmt = format or (ImageFormat.rgb_u8 if c == 3 else ImageFormat.rgba_u8)
        iv = lib.ImageView(w, h, w * c, fmt.value, img.ctypes.data)
        mv = lib.ImageView(msk.shape[1], msk.shape[0], msk.shape[1], ImageFormat.alpha_u8.value, msk.ctypes.data)
        out_view, out_data = lib.ImageView(), c_void_p()
        check(self._api.visp_migan_compute(self._handle, byref(iv), byref(mv), byref(out_view), byref(out_data)))
        return self._take_image(out_view, out_data)

    def compute_batch(self, images: np.ndarray, masks: np.ndarray) -> np.ndarray:
        """images u8 [B, res, res, 3 | 4], masks u8 [B, res, res] -> rgba u8 [B, res, res, 4]."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        msks = np.ascontiguousarray(masks, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert msks.shape == (b, h, w), (msks.shape, imgs.shape)
        out = np.empty((b, h, w, 4), np.uint8)
        check(self._api.visp_migan_compute_batch_host(self._handle, imgs.ctypes.data, c, msks.ctypes.data, b, out.ctypes.data))
        return out

    def compute_batch_device(self, img_dev: int, channels: int, mask_dev: int, batch: int, out_dev: int, stream: int | None = None):
        check(self._api.visp_migan_compute_batch_device(self._handle, img_dev, channels, mask_dev, batch, out_dev, stream))

    def generate(self, x: np.ndarray) -> np.ndarray:
        """migan_process_input's f32 [n, res, res, 4] -> the generator's rgb f32 [n, res, res, 3]."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        out = np.empty(x.shape[:3] + (3,), np.float32)
        check(self._api.visp_migan_generate_host(self._handle, x.ctypes.data, x.shape[0], out.ctypes.data))
        return out


# ---- YOLOv9t (reference src/visp/arch/yolov9t.cpp; loaded through visp_yolov9t_load) --------------

DETECTION_DTYPE = np.dtype([("x1", np.float32), ("y1", np.float32), ("x2", np.float32), ("y2", np.float32), ("confidence", np.float32),
                            ("class_id", np.int32), ("class_confidence", np.float32)])  # == visp_detection (detected_obj)
assert DETECTION_DTYPE.itemsize == ctypes.sizeof(lib.Detection)


def _dets_p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(lib.Detection))


def _nms_params(conf=None, iou=None, max_det=None, max_nms=None, max_wh=None) -> lib.Yolov9tNmsParams:
    """visp_yolov9t_nms_defaults (conf 0.25, iou 0.45, max_det 300, max_nms 30000, max_wh 640) with the given fields replaced."""
    p = lib.Yolov9tNmsParams()
    get_lib().visp_yolov9t_nms_defaults(byref(p))
    for k, v in dict(conf=conf, iou=iou, max_det=max_det, max_nms=max_nms, max_wh=max_wh).items():
        if v is not None:
            setattr(p, k, v)
    return p


def _image_view(image: np.ndarray):
    img = np.ascontiguousarray(image, dtype=np.uint8)
    h, w, c = img.shape
    if c not in (3, 4):
        raise ValueError(f"expected an rgb or rgba u8 image, got {c} channels")
    fmt = ImageFormat.rgb_u8 if c == 3 else ImageFormat.rgba_u8
    return img, lib.ImageView(w, h, w * c, fmt.value, img.ctypes.data)


def yolov9t_letterbox(image: np.ndarray, size: int = 640):
    """letterbox (yolov9t.cpp:1028-1083) on the host: rgb / rgba u8 [h, w, 3|4] -> (rgb u8 [size, size, 3], gain, pad_w, pad_h)."""
    img, view = _image_view(image)
    out = np.empty((size, size, 3), np.uint8)
    gain, pw, ph = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    check(get_lib().visp_yolov9t_letterbox(byref(view), size, out.ctypes.data, byref(gain), byref(pw), byref(ph)))
    return out, gain.value, pw.value, ph.value


def yolov9t_nms(boxes: np.ndarray, scores: np.ndarray, **nms) -> np.ndarray:
    """non_max_suppression (yolov9t.cpp:1145-1253) on the host: boxes f32 [A, 4], scores f32 [A, nc] -> DETECTION_DTYPE [n]."""
    b = np.ascontiguousarray(boxes, np.float32)
    s = np.ascontiguousarray(scores, np.float32)
    a, nc = s.shape
    assert b.shape == (a, 4), (b.shape, s.shape)
    p = _nms_params(**nms)
    out, n = np.empty(p.max_det, DETECTION_DTYPE), c_int32()
    check(get_lib().visp_yolov9t_nms(b.ctypes.data, s.ctypes.data, a, nc, byref(p), _dets_p(out), p.max_det, byref(n)))
    return out[: n.value].copy()


def yolov9t_scale_boxes(dets: np.ndarray, width: int, height: int, gain: float, pad_w: float, pad_h: float) -> np.ndarray:
    """scale_boxes (yolov9t.cpp:1255-1281) on the host: DETECTION_DTYPE boxes in letterbox pixels -> a copy in image pixels."""
    out = np.ascontiguousarray(dets, DETECTION_DTYPE).copy()
    check(get_lib().visp_yolov9t_scale_boxes(_dets_p(out), out.size, width, height, gain, pad_w, pad_h))
    return out


class Yolov9t(Model):
    """YOLOv9t object detection (reference yolov9t.cpp + inference_yolov9t.cpp:300-405). Loaded through visp_yolov9t_load: the
    reference has no model_family for it, so visp_model_load refuses the file."""

    @classmethod
    def load(cls, path, device: Device):
        api = get_lib()
        handle = c_void_p()
        check(api.visp_yolov9t_load(lib.path_to_char_p(path), device._handle, byref(handle)))
        return cls(api, handle, Arch.unknown, device)

    def _family_fn(self, name: str):
        return getattr(self._api, "visp_yolov9t_" + name)

    @property
    def info(self) -> dict:
        i = lib.Yolov9tInfo()
        check(self._api.visp_yolov9t_get_info(self._handle, byref(i)))
        return dict(input_size=i.input_size, num_classes=i.num_classes, reg_max=i.reg_max, n_anchors=i.n_anchors)

    def detect(self, image: np.ndarray, **nms) -> np.ndarray:
        """rgb / rgba u8 [h, w, 3|4] of any extent -> DETECTION_DTYPE [n] in the image's pixels, in score order."""
        img, view = _image_view(image)
        p = _nms_params(**nms)
        out, n = np.empty(p.max_det, DETECTION_DTYPE), c_int32()
        check(self._api.visp_yolov9t_detect(self._handle, byref(view), byref(p), _dets_p(out), p.max_det, byref(n)))
        return out[: min(n.value, p.max_det)].copy()

    def detect_batch(self, images: np.ndarray, **nms) -> list[np.ndarray]:
        """letterboxed u8 [B, S, S, 3|4] -> one DETECTION_DTYPE array per image, in input pixels."""
        imgs = np.ascontiguousarray(images, dtype=np.uint8)
        b, h, w, c = imgs.shape
        assert h == w, imgs.shape
        p = _nms_params(**nms)
        out, counts = np.empty((b, p.max_det), DETECTION_DTYPE), np.zeros(b, np.int32)
        check(self._api.visp_yolov9t_detect_batch_host(self._handle, imgs.ctypes.data, c, b, h, byref(p), _dets_p(out),
                                                       counts.ctypes.data_as(ctypes.POINTER(c_int32))))
        return [out[i, : counts[i]].copy() for i in range(b)]

    def detect_batch_device(self, img_dev: int, channels: int, batch: int, size: int, stream: int | None = None, **nms) -> list[np.ndarray]:
        p = _nms_params(**nms)
        out, counts = np.empty((batch, p.max_det), DETECTION_DTYPE), np.zeros(batch, np.int32)
        check(self._api.visp_yolov9t_detect_batch_device(self._handle, img_dev, channels, batch, size, byref(p), _dets_p(out),
                                                         counts.ctypes.data_as(ctypes.POINTER(c_int32)), stream))
        return [out[i, : counts[i]].copy() for i in range(batch)]

    def detect_batch_resident(self, img_dev: int, channels: int, batch: int, size: int, out_dev: int, counts_dev: int, stream: int | None = None, **nms) -> None:
        """letterboxed u8 [batch, size, size, channels] at device address img_dev -> DETECTION_DTYPE [batch, max_det] at out_dev and i32 [batch] at
        counts_dev, both on the device (rows behind a count are left as they were). Enqueued on `stream`, not synchronised."""
        p = _nms_params(**nms)
        check(self._api.visp_yolov9t_detect_batch_resident(self._handle, img_dev, channels, batch, size, byref(p), out_dev, counts_dev, stream))

    def set_device_nms(self, enable: bool) -> None:
        """detect / detect_batch / detect_batch_device with the NMS on the device: the same detections, only they are read back. Off by default."""
        check(self._api.visp_yolov9t_set_device_nms(self._handle, int(bool(enable))))

    @property
    def last_split(self) -> dict:
        """The last batch call in ms: the launch list on the device (HIP events), the candidate readback, the host NMS; with the device NMS
        on: the launch list and the NMS on the device, the readback of the detections, 0."""
        out = (ctypes.c_float * 3)()
        check(self._api.visp_yolov9t_last_split(self._handle, out))
        return dict(device_ms=out[0], readback_ms=out[1], nms_ms=out[2])

    def forward(self, x: np.ndarray):
        """f32 rgb [n, S, S, 3] in [0, 1] -> (boxes f32 [n, A, 4] xyxy in input pixels, scores f32 [n, A, nc])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        n, s = x.shape[0], x.shape[1]
        a = (s // 8) ** 2 + (s // 16) ** 2 + (s // 32) ** 2
        boxes = np.empty((n, a, 4), np.float32)
        scores = np.empty((n, a, self.info["num_classes"]), np.float32)
        check(self._api.visp_yolov9t_forward_host(self._handle, x.ctypes.data, n, s, boxes.ctypes.data, scores.ctypes.data))
        return boxes, scores
