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

    def sam_generate_masks(self, points_per_side: int = 32, prompts=None, pred_iou_thresh=None, stability_thresh=None, stability_offset=None, nms_iou_thresh=None,
                           max_masks: int = 256, min_mask_region_area: int = 0):
        """SAM's automatic mask generator on the last sam_encode (one crop layer, no crop-edge filter; min_mask_region_area as in SAM: holes and islands below
        that many pixels are removed and a second NMS runs, after which unchanged masks come first and changed ones behind them): the points_per_side^2 grid
        of sam_point_grid, or `prompts` (points and boxes as for sam_compute_batch). Thresholds default to SAM's (sam_generate_defaults). Returns at most
        max_masks records in order of predicted iou, each a dict with SAM's keys: segmentation (bool [h, w]), area, bbox [x, y, w, h] (of the mask, image
        pixels), predicted_iou, stability_score, and point_coords [[x, y]] for a point prompt or box [x0, y0, x1, y1] for a box prompt."""
        p, k, _ = self._sam_generate_args(prompts, points_per_side, pred_iou_thresh, stability_thresh, stability_offset, nms_iou_thresh)
        masks, ii, fi, _ = self.sam_generate_masks_raw([list(q[:c]) for q, c in zip(p, k)], points_per_side, pred_iou_thresh, stability_thresh, stability_offset,
                                                       nms_iou_thresh, max_masks, min_mask_region_area)
        out = []
        for m, row, (piou, stab) in zip(masks, ii, fi):
            prompt = int(row[0])
            rec = dict(segmentation=m == 255, area=int(row[6]), bbox=[int(v) for v in row[2:6]], predicted_iou=float(piou), stability_score=float(stab))
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


def image_scale(image: np.ndarray, width: int, height: int, format: ImageFormat = ImageFormat.rgb_u8) -> np.ndarray:
    """The reference's image_scale (src/visp/image.cpp:328-356) on the host: [h, w, ch] u8 or f32 -> [height, width, ch]."""
    api = lib.get_lib()
    is_f32 = format.value >= ImageFormat.rgba_f32.value
    img = np.ascontiguousarray(image, dtype=np.float32 if is_f32 else np.uint8)
    h, w = img.shape[:2]
    ch = _CHANNELS[format.value]
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

    @property
    def last_split(self) -> dict:
        """The last batch call in ms: the launch list on the device (HIP events), the candidate readback, the host NMS."""
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
