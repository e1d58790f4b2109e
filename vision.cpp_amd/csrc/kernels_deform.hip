// Deformable convolution (nn.cpp:131-148 conv_2d_deform = torchvision deform_conv2d, stride 1) as ONE implicit GEMM on gfx950:
// M = output pixels, N = Cout, K = taps x Cin. The A operand is never stored to HBM: each k step's tile (64 pixels x CK channels of one
// tap) is sampled bilinearly from x straight into LDS, where csrc/birefnet.cpp's composed form writes every sampled column out
// (vx_bf_deform_cols_f16) and reads it back in a GEMM.
//
//  * one block = 64 pixels x ALL of Cout (<= 256): every bilinear sample is taken exactly once. 4 waves; wave w owns the 32-column
//    blocks w and w + 4 of the output for all 64 pixels (2 x 2 accumulators of v_mfma_f32_32x32x16_f16, f32).
//  * offsets (dy, dx per tap) and the mask / modulator logits of the 64 pixels are loaded into LDS once per block.
//  * k step s = (tap, CK-channel chunk). While the MFMAs of step s run on LDS buffer s & 1, the four 16-byte corner loads per 8 channels of
//    step s + 1 are in flight; they are combined (weights f32, the product with the mask rounded to f16 ONCE: the rounding point of
//    bf_deform_cols_kernel) into buffer (s + 1) & 1 behind the MFMAs. One barrier per step.
//  * the weights stream from the packed [Cout pad 32][taps * Cin] f16 image: a wave's B fragments are its own (no other wave reads its
//    columns), so they go global -> registers, one step ahead, and LDS holds A only. A rows are padded by 16 bytes (pitch 2 CK + 16): the
//    ds_read_b128 of 32 rows at one k column is conflict free for every CK.
//  * mask modes: 0 none, 1 the mask tensor as it is, 2 logits (mask_scale * sigmoid(logit) in the sampler). Extension rule: a sample at
//    (py, px) counts only inside (-1, H) x (-1, W), corners outside the map are zero (kernels_birefnet.hip:103-105).
//  * epilogue: optional per-channel scale and bias (a branch's batch norm), ReLU, f16 rows with a leading dimension. A pixel tile that
//    runs past the last pixel computes on the clamped last pixel's rows and does not store them.
#include "vx_common.h"

namespace {

constexpr int DBM = 64; // pixels per block

template <int CK>
__global__ __launch_bounds__(256) void deform_conv_kernel(const vx_deform_conv_args p) {
    constexpr int NCH = CK / 8;           // 16-byte chunks per A row
    constexpr int PITCH = CK * 2 + 16;    // bytes per A row in LDS
    constexpr int NKS = CK / 16;          // MFMA k steps per tile
    constexpr int ITEMS = DBM * NCH;      // (pixel, 8-channel chunk) samples per tile
    constexpr int IPT = (ITEMS + 255) / 256;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    f16* const s_om = reinterpret_cast<f16*>(smem + 2 * DBM * PITCH); // [DBM][3 taps]: dy, dx per tap, then the mask values / logits

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int k = p.k, taps = k * k, H = p.H, W = p.W, Cin = p.Cin;
    const int OH = H + 2 * p.pad - k + 1, OW = W + 2 * p.pad - k + 1;
    const int M = p.B * OH * OW, m0 = blockIdx.x * DBM;
    const int Ktot = taps * Cin, nsteps = Ktot / CK;
    const int nblk = (p.Cout + 31) >> 5;
    const bool has[2] = {wave < nblk, wave + 4 < nblk};

    const f16* __restrict__ xg = reinterpret_cast<const f16*>(p.x);
    const f16* __restrict__ wg = reinterpret_cast<const f16*>(p.w);
    {
        const f16* __restrict__ og = reinterpret_cast<const f16*>(p.offset);
        const f16* __restrict__ mg = reinterpret_cast<const f16*>(p.mask);
        const int per = 3 * taps;
        for (int i = tid; i < DBM * per; i += 256) {
            const int row = i / per, j = i - row * per;
            const long m = min(m0 + row, M - 1);
            s_om[i] = j < 2 * taps ? og[m * p.ld_offset + j] : (p.mask_mode ? mg[m * p.ld_mask + (j - 2 * taps)] : (f16)1);
        }
    }

    // the samples of this thread: the same (pixel, chunk) in every step
    int it_row[IPT], it_ch[IPT], it_oy[IPT], it_ox[IPT];
    const f16* it_base[IPT];
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const int i = tid + j * 256;
        it_row[j] = i < ITEMS ? i / NCH : -1;
        it_ch[j] = i % NCH;
        const int m = min(m0 + max(it_row[j], 0), M - 1);
        const int b = m / (OH * OW), rm = m - b * (OH * OW);
        it_oy[j] = rm / OW - p.pad;
        it_ox[j] = rm % OW - p.pad;
        it_base[j] = xg + (long)b * H * W * Cin + it_ch[j] * 8;
    }
    __syncthreads(); // s_om

    f16x8 cv[IPT][4]; // corner values of the step in flight
    float cw[IPT][5]; // their weights, and the mask factor
    auto fetch = [&](int s) {
        const int cpt = Cin / CK, tap = s / cpt, c0 = (s - tap * cpt) * CK;
        const int ky = tap / k, kx = tap - ky * k;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            cv[j][0] = cv[j][1] = cv[j][2] = cv[j][3] = z;
            cw[j][0] = cw[j][1] = cw[j][2] = cw[j][3] = cw[j][4] = 0.0f;
            if (it_row[j] < 0) continue;
            const f16* o = s_om + it_row[j] * 3 * taps;
            const float py = (float)(it_oy[j] + ky) + (float)o[2 * tap], px = (float)(it_ox[j] + kx) + (float)o[2 * tap + 1];
            if (py > -1.0f && py < (float)H && px > -1.0f && px < (float)W) {
                const float mv = (float)o[2 * taps + tap];
                cw[j][4] = p.mask_mode == 2 ? p.mask_scale / (1.0f + __expf(-mv)) : mv;
                const int y0 = (int)floorf(py), x0 = (int)floorf(px);
                const float ly = py - (float)y0, lx = px - (float)x0;
                const f16* base = it_base[j] + c0;
                if (y0 >= 0 && x0 >= 0) cv[j][0] = *reinterpret_cast<const f16x8*>(base + ((long)y0 * W + x0) * Cin);
                if (y0 >= 0 && x0 + 1 <= W - 1) cv[j][1] = *reinterpret_cast<const f16x8*>(base + ((long)y0 * W + x0 + 1) * Cin);
                if (y0 + 1 <= H - 1 && x0 >= 0) cv[j][2] = *reinterpret_cast<const f16x8*>(base + ((long)(y0 + 1) * W + x0) * Cin);
                if (y0 + 1 <= H - 1 && x0 + 1 <= W - 1) cv[j][3] = *reinterpret_cast<const f16x8*>(base + ((long)(y0 + 1) * W + x0 + 1) * Cin);
                cw[j][0] = (1.0f - ly) * (1.0f - lx); cw[j][1] = (1.0f - ly) * lx; cw[j][2] = ly * (1.0f - lx); cw[j][3] = ly * lx;
            }
        }
    };
    auto finish = [&](int buf) {
        unsigned char* const sa = smem + buf * DBM * PITCH;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if (it_row[j] < 0) continue;
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                o[e] = (f16)((cw[j][0] * (float)cv[j][0][e] + cw[j][1] * (float)cv[j][1][e] + cw[j][2] * (float)cv[j][2][e] + cw[j][3] * (float)cv[j][3][e]) * cw[j][4]);
            *reinterpret_cast<f16x8*>(sa + it_row[j] * PITCH + it_ch[j] * 16) = o;
        }
    };

    f16x8 bcur[2][NKS] = {}, bnext[2][NKS] = {};
    auto load_b = [&](int s, f16x8 (&bf)[2][NKS]) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            if (!has[ni]) continue;
            const f16* row = wg + (long)((wave + 4 * ni) * 32 + r) * Ktot + (long)s * CK + h * 8;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) bf[ni][ks] = *reinterpret_cast<const f16x8*>(row + ks * 16);
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.0f;

    fetch(0);
    load_b(0, bcur);
    finish(0);
    __syncthreads();
    for (int s = 0; s < nsteps; ++s) {
        const bool more = s + 1 < nsteps;
        if (more) {
            fetch(s + 1);
            load_b(s + 1, bnext);
        }
        __builtin_amdgcn_sched_barrier(0); // the next step's loads are issued before this step's MFMAs
        const unsigned char* const sa = smem + (s & 1) * DBM * PITCH + r * PITCH + h * 16;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            f16x8 af[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) af[mi] = *reinterpret_cast<const f16x8*>(sa + mi * 32 * PITCH + ks * 32);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) {
                if (!has[ni]) continue;
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bcur[ni][ks], af[mi], acc[mi][ni], 0, 0, 0);
            }
        }
        if (more) {
            finish((s + 1) & 1);
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) bcur[ni][ks] = bnext[ni][ks];
        }
        __syncthreads(); // buffer (s + 1) & 1 is written; every wave is done reading buffer s & 1
    }

    // a lane owns pixel row mi * 32 + r and, per register group g, the 4 consecutive channels 8 g + 4 h .. + 3 of its column blocks
    f16* const out = reinterpret_cast<f16*>(p.out);
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int m = m0 + mi * 32 + r;
        if (m >= M) continue;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            if (!has[ni]) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = (wave + 4 * ni) * 32 + 8 * g + 4 * h;
                if (n >= p.Cout) continue;
                float v[4] = {acc[mi][ni][4 * g], acc[mi][ni][4 * g + 1], acc[mi][ni][4 * g + 2], acc[mi][ni][4 * g + 3]};
                if (p.scale) {
                    const float4 sc = *reinterpret_cast<const float4*>(p.scale + n);
                    v[0] *= sc.x; v[1] *= sc.y; v[2] *= sc.z; v[3] *= sc.w;
                }
                if (p.bias) {
                    const float4 bi = *reinterpret_cast<const float4*>(p.bias + n);
                    v[0] += bi.x; v[1] += bi.y; v[2] += bi.z; v[3] += bi.w;
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
                }
                const f16x4 o = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
                *reinterpret_cast<f16x4*>(out + (long)m * p.ldo + n) = o;
            }
        }
    }
}

template <int CK>
void launch_deform(const vx_deform_conv_args& a, int blocks, int taps, hipStream_t st) {
    const size_t lds = (size_t)2 * DBM * (CK * 2 + 16) + (size_t)DBM * 3 * taps * 2;
    hipLaunchKernelGGL(deform_conv_kernel<CK>, dim3(blocks), dim3(256), lds, st, a);
}

} // namespace

extern "C" int vx_deform_conv_f16(const vx_deform_conv_args* a, void* stream) {
    VX_REQUIRE(a && a->x && a->w && a->offset && a->out, "vx_deform_conv_f16: null operand");
    VX_REQUIRE(a->B > 0 && a->H > 0 && a->W > 0 && a->Cin > 0 && a->Cin % 16 == 0, "vx_deform_conv_f16: Cin = %d must be a multiple of 16", a->Cin);
    VX_REQUIRE(a->Cout > 0 && a->Cout <= 256 && a->Cout % 8 == 0, "vx_deform_conv_f16: Cout = %d (a multiple of 8, at most 256: one block computes all of it)", a->Cout);
    VX_REQUIRE(a->k >= 1 && a->k <= 7 && a->pad >= 0, "vx_deform_conv_f16: kernel %d, pad %d (kernels 1..7)", a->k, a->pad);
    const int taps = a->k * a->k;
    const long OH = (long)a->H + 2 * a->pad - a->k + 1, OW = (long)a->W + 2 * a->pad - a->k + 1;
    VX_REQUIRE(OH > 0 && OW > 0 && (long)a->B * OH * OW < (1l << 31) - 64, "vx_deform_conv_f16: output extent %ldx%ld", OW, OH);
    VX_REQUIRE((long)a->B * a->H * a->W * a->Cin < (1l << 40), "vx_deform_conv_f16: input too large");
    VX_REQUIRE(a->ld_offset >= 2 * taps, "vx_deform_conv_f16: offset rows of %d elements hold fewer than 2 x %d taps", a->ld_offset, taps);
    VX_REQUIRE(a->mask_mode >= 0 && a->mask_mode <= 2 && (a->mask_mode == 0 || (a->mask && a->ld_mask >= taps)),
               "vx_deform_conv_f16: mask mode %d (0 none, 1 mask, 2 logits) with mask rows of %d elements for %d taps", a->mask_mode, a->ld_mask, taps);
    VX_REQUIRE(a->ldo >= a->Cout && a->ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(a->out) & 7) == 0, "vx_deform_conv_f16: output rows of %d elements (>= Cout, a multiple of 4, 8-byte aligned)", a->ldo);
    VX_REQUIRE(aligned16(a->x) && aligned16(a->w) && (!a->scale || aligned16(a->scale)) && (!a->bias || aligned16(a->bias)), "vx_deform_conv_f16: x, w, scale and bias must be 16-byte aligned");
    const int blocks = (int)(((long)a->B * OH * OW + DBM - 1) / DBM);
    hipStream_t st = as_stream(stream);
    if (a->Cin % 64 == 0) launch_deform<64>(*a, blocks, taps, st);
    else if (a->Cin % 48 == 0) launch_deform<48>(*a, blocks, taps, st);
    else if (a->Cin % 32 == 0) launch_deform<32>(*a, blocks, taps, st);
    else launch_deform<16>(*a, blocks, taps, st);
    VX_LAUNCH_CHECK();
    return 1;
}
