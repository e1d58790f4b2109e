"""The case table of tests/test_gpu_gemm_matrix.py, kept apart from it so that tests/test_gemm_ref_cpu.py can check it for completeness
without a device. A case is a dict of vx_gemm_args fields (scalars only) plus three bookkeeping keys: `id`, `group` (a / b / c of the
table below) and `form` (the block-tile form the dispatcher picks for it). Keys that start with `_` tell `materialize` which optional
operands to generate. `materialize(case)` adds the seeded operand arrays and returns the argument dict tests/gemm_ref.py evaluates.

  a. every epilogue on every block-tile form, plain mode, K = 64, M = 2 * BM + 77 (the tail tile has waves without a valid row)
  b. split-K, plain and implicit conv, even and uneven k ranges, the three tile widths, n_valid < ldo
  c. implicit-conv geometry: kernel extents, strides, pads, K padded past kh*kw*Cin, channel-slice reads, ReLU on load"""
from __future__ import annotations

import zlib

import numpy as np

from gemm_ref import ADD, F16, GELU, HEAD_OUT, LRELU_AGC, PIXSHUF, QKV, RELU, RESID_F32, SILU, TOKENS

# form -> (vx_gemm_args.stages, N granularity that reaches it, block-tile rows)
FORMS = {
    "128x128": (0, 128, 128),
    "128x128s2": (2, 128, 128),
    "256x128w4": (4, 128, 256),
    "256x128w8": (8, 128, 256),
    "128x64": (16, 128, 128),
    "128x128w8": (32, 128, 128),
    "192x128": (64, 128, 192),
    "n64": (0, 64, 128),   # N % 128 != 0, N % 64 == 0: 128x64 by N alone (N = 192)
    "n32": (0, 32, 128),   # N % 64 != 0: 128x32 (N = 96)
}
CONV_EPILOGUES = (F16, GELU, RELU, ADD, HEAD_OUT, SILU)  # dispatch_epi<true>


def forms_of(epi):
    """the tile forms an epilogue can be dispatched on: HEAD_OUT is N == 32 only, QKV needs N = 3 * H * 64 (a multiple of 64)"""
    if epi == HEAD_OUT:
        return {"n32"}
    return set(FORMS) - ({"n32"} if epi == QKV else set())


def _round_up(x, m):
    return -(-x // m) * m


def _plain_variants(form):
    """(name, fields) of group a for one tile form; N / M are filled in by the caller unless set here"""
    gran = FORMS[form][1]
    n_of = {128: 128, 64: 192, 32: 96}[gran]
    v = [
        ("f16", dict(epi=F16, _lda_pad=8, _ldo_pad=8)),
        ("f16_rowremap", dict(epi=F16, a_group=50, a_group_stride=51, a_row_off=1)),
        ("gelu", dict(epi=GELU)),
        ("relu", dict(epi=RELU)),
        ("resid", dict(epi=RESID_F32)),  # lambda ~ N(0, 0.3): mixed sign
        ("tokens_P37", dict(epi=TOKENS, tokens_P=37)),
        ("tokens_P200", dict(epi=TOKENS, tokens_P=200)),
        ("add", dict(epi=ADD)),
        ("add_res1", dict(epi=ADD, _res1=1)),
        ("add_res1_res2", dict(epi=ADD, _res1=1, _res2=1)),
        ("add_relu", dict(epi=ADD, relu=1, _res1=1)),
        ("add_post_gelu", dict(epi=ADD, post_gelu=1, _res1=1)),
        # window_reverse + residual: 7x7 windows on a 9 wide x 8 high map (2 x 2 windows per image), B = 3 -> M = 3 * 4 * 49 = 588
        ("add_win_shift0", dict(epi=ADD, win_ws=7, win_res=9, win_res_h=8, win_shift=0, M=588, _res1=1)),
        ("add_win_shift3", dict(epi=ADD, win_ws=7, win_res=9, win_res_h=8, win_shift=3, M=588, _res1=1, _res2=1)),
        # bias spikes of +-2000 put whole columns on the clamp of +-256; noise_hw = 45 divides none of the tile heights
        ("lrelu", dict(epi=LRELU_AGC, _spikes=1)),
        ("lrelu_noise", dict(epi=LRELU_AGC, _spikes=1, _noise=1, noise_hw=45)),
        ("lrelu_noise_res1", dict(epi=LRELU_AGC, _spikes=1, _noise=1, noise_hw=45, _res1=1)),
        ("silu", dict(epi=SILU)),
        ("silu_res1", dict(epi=SILU, _res1=1, _ld_res1_pad=16)),
    ]
    # pixel shuffle: N = s * s * Cout padded to the form's granularity, 5 x 7 input maps, the last image partial
    ps = {128: [(2, 32, 128), (4, 8, 128)], 64: [(2, 48, 192), (4, 8, 192)], 32: [(2, 24, 96), (4, 8, 160)]}[gran]
    for s, co, n in ps:
        v.append((f"pixshuf_s{s}", dict(epi=PIXSHUF, ps_s=s, ps_Cout=co, ps_H=5, ps_W=7, N=n, n_valid=s * s * co, ldo=co)))
    if form in forms_of(QKV):
        # T = 50: more than two images per tile; 150: >= 128 but below the tall tiles (the division fallback); 257: a tile straddles two images
        heads = 1 if gran == 64 else 2
        for T in (50, 150, 257):
            v.append((f"qkv_T{T}", dict(epi=QKV, qkv_T=T, qkv_H=heads, q_scale=0.125, N=3 * heads * 64)))
    if form == "n32":
        v.append(("head_out", dict(epi=HEAD_OUT, N=32, head_bias=0.05, head_scale=2.0, ldo=1)))
    return [(name, dict(dict(N=n_of), **f)) for name, f in v]


def _group_a():
    cases = []
    for form, (stages, _, bm) in FORMS.items():
        for name, f in _plain_variants(form):
            c = dict(id=f"a-{name}-{form}", group="a", form=form, M=2 * bm + 77, K=64, stages=stages)
            c.update(f)
            cases.append(c)
    # the default dispatcher picks 192x128 by its own formula: N / 128 = 12 column tiles; 128-row tiles: ceil(10881 / 128) = 86 -> 1032 tiles,
    # 2 rounds of the 1024 resident slots -> cost 2 * 128 = 256; 192-row tiles: ceil(10881 / 192) = 57 -> 684 tiles, 1 round of 768 -> cost 192
    cases.append(dict(id="a-f16-dispatcher-picks-192x128", group="a", form="192x128", epi=F16, M=10881, N=1536, K=64, stages=0))
    return cases


def _conv_fields(kh, kw, stride, pad, cin, B, H, W):
    OH, OW = (H + 2 * pad - kh) // stride + 1, (W + 2 * pad - kw) // stride + 1
    return dict(conv_kh=kh, conv_kw=kw, conv_stride=stride, conv_pad=pad, conv_H=H, conv_W=W, conv_Cin=cin, conv_OH=OH, conv_OW=OW,
                M=B * OH * OW, K=_round_up(kh * kw * cin, 64), _B=B)


def _group_b():
    cases = []
    epis = [("f16", dict(epi=F16)), ("relu", dict(epi=RELU)), ("add", dict(epi=ADD, _res1=1)), ("add_relu", dict(epi=ADD, relu=1, _res1=1))]
    form_of_n = {64: "n64", 128: "128x128", 96: "n32"}
    # plain: K = 1280 is 20 k-tiles; 2 -> 10 + 10, 3 -> 7 + 7 + 6, 7 -> six ranges of 3 and one of 2
    for ks in (2, 3, 7):
        for n in (64, 128, 96):
            for name, f in epis:
                cases.append(dict(dict(id=f"b-plain-{name}-N{n}-ks{ks}", group="b", form=form_of_n[n], M=200, N=n, K=1280, k_splits=ks), **f))
    for name, f in epis:
        cases.append(dict(dict(id=f"b-plain-{name}-nvalid40-ldo48", group="b", form="n64", M=200, N=64, K=1280, k_splits=3, n_valid=40, ldo=48), **f))
    # implicit conv 3x3, Cin = 256 on a 9 x 13 map: K = 2304 is 36 k-tiles; 5 -> four ranges of 8 and one of 4 (7 would leave an empty range)
    for ks in (2, 3, 5):
        for n in (64, 128, 96):
            for name, f in epis:
                c = dict(id=f"b-conv-{name}-N{n}-ks{ks}", group="b", form=form_of_n[n], N=n, k_splits=ks)
                c.update(_conv_fields(3, 3, 1, 1, 256, 2, 9, 13))
                c.update(f)
                cases.append(c)
    return cases


GEOMETRIES = [(1, 1, 2, 0), (3, 3, 1, 1), (3, 3, 2, 1), (5, 5, 1, 2), (7, 7, 1, 3), (3, 1, 1, 1), (1, 3, 1, 0), (3, 3, 1, 0)]  # kh, kw, stride, pad


def _group_c():
    cases = []
    epis = [
        ("gelu", "128x128", dict(epi=GELU, N=128)),
        ("relu", "n32", dict(epi=RELU, N=96)),
        ("add", "n64", dict(epi=ADD, N=64, relu=1, _res1=1, _res2=1)),
        ("silu", "n64", dict(epi=SILU, N=64, _res1=1, _ld_res1_pad=16)),
        ("head_out", "n32", dict(epi=HEAD_OUT, N=32, head_bias=0.05, head_scale=2.0, ldo=1)),
    ]
    for kh, kw, stride, pad in GEOMETRIES:
        for cin in (8, 24, 64):
            for H, W in ((11, 7), (10, 10)):  # B = 2: the second image starts inside a 128-row tile
                geo = _conv_fields(kh, kw, stride, pad, cin, 2, H, W)
                tag = f"{kh}x{kw}s{stride}p{pad}-c{cin}-{H}x{W}"
                cases.append(dict(dict(id=f"c-f16-{tag}", group="c", form="n64", epi=F16, N=64), **geo))
                if (kh, kw) not in ((3, 3), (7, 7)):
                    continue
                for name, form, f in epis:
                    for vname, vf in (("", {}), ("-arelu", dict(a_relu=1)), ("-slice", dict(conv_pix=cin + 16, _A_off=8))):
                        c = dict(id=f"c-{name}{vname}-{tag}", group="c", form=form)
                        c.update(geo)
                        c.update(f)
                        c.update(vf)
                        cases.append(c)
    return cases


CASES = _group_a() + _group_b() + _group_c()
assert len({c["id"] for c in CASES}) == len(CASES)


def group(name):
    return [c for c in CASES if c["group"] == name]


def materialize(case):
    """case -> argument dict with every operand array (seeded by the case id) and the defaulted lda / ldo"""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    a = {k: v for k, v in case.items() if not k.startswith("_") and k not in ("id", "group", "form")}
    M, N, K, epi = a["M"], a["N"], a["K"], a["epi"]

    def normal(*shape, scale=1.0, dtype=np.float16):
        return (rng.standard_normal(shape) * scale).astype(dtype)

    if a.get("conv_kh", 0) > 0:
        pix = a.get("conv_pix") or a["conv_Cin"]
        a["A"] = normal(case["_B"], a["conv_H"], a["conv_W"], pix)  # the channels outside the slice hold values too
        a["A_off"] = case.get("_A_off", 0)
        k_real = a["conv_kh"] * a["conv_kw"] * a["conv_Cin"]
    else:
        a["lda"] = K + case.get("_lda_pad", 0)
        g = a.get("a_group", 0)
        rows = M if g <= 0 else -(-M // g) * a["a_group_stride"] + a["a_row_off"]
        a["A"] = normal(rows, a["lda"])
        k_real = K
    # the K padding of W is NOT zero here: in conv mode the loader itself must zero-fill A past kh*kw*Cin
    a["W"] = normal(N, K, scale=k_real ** -0.5)
    bias = normal(N, scale=0.1, dtype=np.float32)
    if case.get("_spikes"):
        bias[3::16], bias[11::16] = 2000.0, -2000.0
        a["A"] = (a["A"].astype(np.float32) * 200).astype(np.float16)  # z ~ N(0, 200): the upper clamp is hit by data as well
    a["bias"] = bias
    a.setdefault("ldo", N + case.get("_ldo_pad", 0))
    ldo = a["ldo"]
    from gemm_ref import out_rows
    n_rows = out_rows(a)
    if case.get("_res1"):
        ld = ldo + case.get("_ld_res1_pad", 0)
        if ld != ldo:
            a["ld_res1"] = ld
        a["res1"] = normal(n_rows, ld)
    if case.get("_res2"):
        a["res2"] = normal(n_rows, ldo)
    if case.get("_noise"):
        a["noise"] = normal(a["noise_hw"], dtype=np.float32)
    if epi in (RESID_F32, HEAD_OUT):
        a["lambda_"] = normal(N, scale=0.3, dtype=np.float32)
    if epi == RESID_F32:
        a["out0"] = normal(M, ldo, dtype=np.float32)
    if epi == TOKENS:
        a["pos"] = normal(a["tokens_P"] + 1, N, dtype=np.float32)
    return a
