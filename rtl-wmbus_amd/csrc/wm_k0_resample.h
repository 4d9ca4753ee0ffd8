/*
 * wm_k0_resample.h -- K0: exact integer rational resampler in front of the demodulation kernel (cfg.input_rate_hz).
 *
 * The reference takes captures at a multiple of 800 kHz only (rtl_wmbus.c:1274-1292: "use a multiple of 800kHz").  K0 turns a cu8
 * capture at any rate Fin with Fout / Fin = L / M (L <= 32, M <= 1024) into an ordinary cu8 stream at Fout = decimation x 800 kHz in
 * the context's device input window; K1 and everything behind it run unchanged on that stream.
 *
 * The arithmetic is the definition (include/wmbus_hip.h, wmbus_resampler_design; tests/resample_ref.py restates it in numpy):
 *   x = 2u - 255 per byte; history before the stream's first sample is x = 0
 *   output n: phase p = (n M) mod L, newest input b = floor(n M / L), acc = sum_{k < T} taps[p][k] x[b - k]      (int32, exact)
 *   byte = clamp((acc + 255 * 16384 + 16384) >> 15, 0, 255)
 * Pure integers: nothing here depends on a float, so the bytes do not depend on tile, block or push boundaries.
 *
 * Shape: block = (tile of consecutive outputs, capture).  The input span of the tile (tile M / L + T samples) goes once into LDS
 * as one dword per sample, {I, Q} as two int16, loaded with aligned dword loads of two samples; the L x T int16 taps sit beside
 * it.  A lane owns K0_OPL outputs of ONE phase (n, n + L, n + 2L, ...: their newest inputs lie exactly M apart), so a dword of two
 * taps is read once for all of them; per tap pair and output two sample dwords are read, V_PERM_B32 regroups them into {I, I'} and
 * {Q, Q'} and V_DOT2_I32_I16 does the two multiply-adds of each.  The bytes are gathered in LDS and leave as 16-bit vector stores
 * of consecutive lanes (the window position of a push's first byte is even, not dword aligned: it follows the remainder).
 *
 * Carried from push to push, per capture, all on the device and double-buffered like every other carried state: the last T - 1
 * samples (as {I, Q} int16 pairs) and the bytes behind the last whole 4096-byte block (the pipeline takes whole blocks, as the
 * reference's fread does).  The output counter is the same for every capture of a context (they advance in lock step) and
 * travels as a launch argument, like WmPush.n0.
 *
 * Sample formats and input gain (cfg.input_format, cfg.input_gain_q8; the contract is in include/wmbus_hip.h): the format is a
 * template parameter of the block function.  Only the staging loop that fills the LDS span (and the history hand-over) knows the
 * raw layout -- every format becomes the same {I, Q} int16 pair there -- and only the output stage knows the shift F and the gain:
 *   cu8  x = 2u - 255   cs8  x = 2s + 1 (one XOR in front of the cu8 rule)   F = 15
 *   cs16 x = s (the raw dword IS the LDS dword)   cf32 x = clamp(rint(f 32768)), NaN -> 0   F = 22
 *   byte = clamp((acc g + (128 << (F + 8))) >> (F + 8), 0, 255), the product in int64; g = 256 at F = 15 is the line above.
 * k0_convert_block is the same stage for an input that is already at decimation x 800 kHz (acc = 16384 x): no taps, no LDS span,
 * 16 raw bytes per lane and load, the same remainder / keep_from hand-over.  Both count the bytes the clamp changed (K0Args.clipped):
 * per lane in a register, per block in LDS, one atomic add per block.
 *
 * Frequency shift (cfg.input_shift_hz; the contract is in include/wmbus_hip.h): the second template parameter SH of both block
 * functions.  Every input sample is rotated ONCE, where it is staged -- behind k0_load2 in the loop that fills the LDS span and in
 * the history hand-over (the carried history holds rotated samples), between the 16-byte load and k0_byte_g in k0_convert_block --
 * by the table entry of its phase (step m) mod 2^32, m = in_first + its index within the push: a function of m alone, nothing
 * carried.  One dword {c, s} per entry from the 4 KB table in global memory (K0Args.shift_tab; DESIGN.md section 4 says why not LDS),
 * {-s, c} built from it with V_PERM_B32, one V_DOT2_I32_I16 per component.  cu8 / cs8 samples are widened to 64 x first and F is
 * 21 instead of 15.  SH = false compiles to exactly the code there was: every line of the shift sits behind if constexpr (SH).
 *
 * I/Q DC blocker (cfg.input_dc = R; the contract is in include/wmbus_hip.h): the third template parameter DC of both block functions,
 * and two small kernels in front of them.  k0_dc_sums adds up x per level block of 512 input samples (one wave per block, 16-byte
 * loads, the wave reduced with __shfl_xor); k0_dc_plan walks the push's blocks in order -- A[k] = A[k-1] - (A[k-1] >> R) + S[k] is
 * sequential by definition: one wave per component, on the scalar unit -- from the carried {A_I, A_Q, started} of the stream and leaves
 * one dword {dc_I, dc_Q} per block in K0Args.dc_tab.  The block functions subtract it, saturating, where a sample is staged: in front of k0_x64 and the rotation, in the
 * loop that fills the LDS span, in the history hand-over (the carried history holds x') and in k0_convert_block.  The two samples of
 * a k0_load2 and the samples of a conversion lane's 16 bytes share a level block (index within the push >> 9): one table read per
 * group.  DC = false compiles to exactly the code there was: every line of the blocker sits behind if constexpr (DC).
 *
 * Per-block AGC (cfg.input_agc; the contract is in include/wmbus_hip.h): the fourth template parameter AG of both block functions, and
 * one small kernel in front of them, behind the blocker's two where there is a blocker (it needs x').  k0_agc_gain takes the peak
 * P = max(|x'_I| + |x'_Q|) of each level block -- one wave per block, 16-byte loads, the wave reduced with __shfl_xor -- and leaves
 * g = clamp(floor((96 << U) / max(P, 1)), 1, 65535) per block as one uint16 in K0Args.agc_tab.  It is stateless: FSK has a constant
 * envelope, a block's own peak is the estimate, nothing is carried.  The output stage takes g from the table instead of cfg.input_gain_q8:
 * k0_convert_block once per lane group (its samples share a level block, as they share dc), the resampler per output, from the level
 * block of that output's newest input sample.  g differs from lane to lane, so the product is always the 64-bit one.  AG = false compiles
 * to exactly the code there was: every line of the AGC sits behind if constexpr (AG).
 *
 * Channels (cfg.input_channels = C; the contract is in include/wmbus_hip.h): the fifth template parameter CH of both block functions.  One
 * raw capture feeds C pipeline streams, each with a phase step of its own.  The grid stays (tile, pipeline stream): blockIdx.y = v =
 * capture * C + channel, and everything a stream carries -- history, remainder, output window -- is indexed by v as it always was.  The
 * raw pointer and the rows of dc_tab / agc_tab come from capture v / C, the step from K0Args.steps[v % C]: ONE division per block, on the
 * scalar unit (C is a launch argument), none per sample.  The rotation is always on in this form (a 0 Hz channel is step 0, table entry
 * 0 = {16384, 0}: the bytes of the unshifted rule), so CH implies SH; every block stages its own span -- C blocks read a capture's span
 * C times, from L2 after the first (DESIGN.md section 6 has the numbers and the form that stages once).  k0_dc_sums, k0_dc_plan and
 * k0_agc_gain run in front of the rotation: they launch over captures.  In this form the blocker and the AGC are block-uniform runtime
 * branches (dc_tab / agc_tab given or not) instead of instantiations of their own.  CH = false compiles to exactly the code there was:
 * every line of the channels form sits behind if constexpr (CH), and DCX / AGX / dc_on / ag_on are then the constants DC and AG.
 *
 * AFC (cfg.input_afc; the contract is in include/wmbus_hip.h, the plan kernel in wm_k0_afc.h): the sixth template parameter AF of both block
 * functions.  The phase step is no longer a constant of the context: k0_afc_plan, launched in front of the stage kernel of the same push,
 * leaves {step, base} per capture in K0Args.afc, and sample j of the PUSH is rotated by the entry of phase base + step j -- the same
 * k0_rotate, a push-local index in the place of the stream's, base in the place of 0.  k0_capture_of and k0_shifted are the two places
 * that know.  AF implies SH; like the channels form it takes the blocker and the AGC as runtime branches (one instantiation per format
 * and stage).  AF = false compiles to exactly the code there was: base is the constant 0 and m_first the stream's index.
 * CH and AF together (cfg.input_channel_afc_hz: a lock per channel): the capture is v / n_ch as in the channels form, {step, base} are
 * K0Args.afc[v] -- k0_afc_plan has run once per pipeline stream v, a fixed channel's entry is its own step and the phase that runs on --
 * and K0Args.steps is not looked at.
 */
#ifndef WM_K0_RESAMPLE_H
#define WM_K0_RESAMPLE_H

#include <math.h>
#include <stdint.h>

#define WM_K0_THREADS   256u
#define WM_K0_OPL       4u         /* outputs of one phase per lane */
#define WM_K0_MAX_L     32u
#define WM_K0_MAX_M     1024u
#define WM_K0_MAX_T     512u
#define WM_K0_OUT_BIAS  (255 * 16384 + 16384)
#define WM_K0_CU8   0              /* = WMBUS_FMT_* of include/wmbus_hip.h */
#define WM_K0_CS8   1
#define WM_K0_CS16  2
#define WM_K0_CF32  3
#define WM_K0_CONV_UNROLL 4u       /* k0_convert_block: 16-byte loads a lane has in flight */
#define WM_K0_DC_LOG2   9u         /* a level block of the DC blocker: 512 input samples */
#define WM_K0_DC_MAX_R  12u
#define WM_K0_AGC_TARGET 96u       /* a level block's peak |I| + |Q| lands on +-96 of the byte's +-127 */
#define WM_K0_MAX_CH    8u         /* = WMBUS_MAX_CHANNELS of include/wmbus_hip.h */

/* AFC (wm_k0_afc.h): what k0_afc_plan leaves the stage kernel about one capture and one push */
struct K0AfcPush { uint32_t step, base; };     /* the phase advance per input sample; the phase of the push's first sample */

struct K0Args {
    const uint8_t *raw;         /* [S][raw_stride] the raw cu8 of this push                                  */
    uint64_t raw_stride;
    uint8_t *out;                /* [S][out_stride] first byte behind the window's history                    */
    uint64_t out_stride;
    const int16_t *taps;         /* [L][T]                                                                    */
    const uint32_t *hist_in;     /* [S][T - 1] the T - 1 samples in front of this push, {I, Q} int16          */
    uint32_t *hist_out;          /* the same for the next push                                                */
    const uint8_t *rem_in;       /* [S][4096] bytes produced by earlier pushes and not yet handed on          */
    uint8_t *rem_out;
    uint64_t n_first;            /* output counter at the start of this push                                  */
    uint64_t in_first;           /* input samples of earlier pushes                                           */
    uint32_t n_in, n_out;        /* input samples / outputs of this push                                      */
    uint32_t rem_prev;           /* bytes in rem_in                                                           */
    uint32_t keep_from;          /* window bytes from here on wait for the next push: they go to rem_out too  */
    uint32_t L, M, T, tile;      /* tile: outputs per block (even)                                            */
    /* sample formats and gain; all zero: cu8, gain x 1, nothing counted */
    uint32_t gain_q8;            /* cfg.input_gain_q8 (0: 256)                                                */
    uint32_t *clipped;           /* += output bytes the clamp changed in this push, all captures (NULL: not counted) */
    /* frequency shift (the SH instantiations only); all zero: none */
    uint32_t step;               /* phase advance per input sample, 2^32 = one turn                           */
    const uint32_t *shift_tab;   /* [1024] {c, s} int16: rint(16384 cos / sin(2 pi i / 1024))                 */
    /* I/Q DC blocker (the DC instantiations only); all zero: none */
    const uint32_t *dc_tab;      /* [S][dc_stride] {dc_I, dc_Q} int16 of this push's level blocks (k0_dc_plan) */
    uint32_t dc_stride;          /* level blocks per capture in dc_tab and agc_tab                            */
    /* per-block AGC (the AG instantiations only); NULL: none */
    const uint16_t *agc_tab;     /* [S][dc_stride] g of this push's level blocks (k0_agc_gain): takes gain_q8's place */
    /* channels (the CH instantiations only); all zero: none.  With channels out, hist and rem are [S = captures x n_ch] rows, row v =
     * capture * n_ch + channel; raw, dc_tab and agc_tab stay [captures] */
    uint32_t n_ch;               /* channels per capture                                                      */
    uint32_t steps[WM_K0_MAX_CH];/* the phase step of each channel: takes step's place                        */
    /* AFC (the AF instantiations only); NULL: none */
    const K0AfcPush *afc;        /* [S] this push's {step, base} of every capture (k0_afc_plan): take step's place; the sample index is push-local.
                                    With channels (CH && AF): of every pipeline stream v = capture * n_ch + channel */
};

/* the carried state of the DC blocker, per capture */
struct alignas(8) K0DcState { int64_t a_i, a_q; uint64_t started; };
struct alignas(8) K0S2 { int32_t i, q; };
/* k0_dc_sums and k0_dc_plan: what they read and leave for a push of n_blk level blocks per capture */
struct K0DcArgs {
    const uint8_t *raw;          /* [S][raw_stride] the raw bytes of this push                                */
    uint64_t raw_stride;
    K0S2 *sums;                  /* [S][stride] sum of x over each level block                                */
    uint32_t *tab;               /* [S][stride] K0Args.dc_tab                                                 */
    const K0DcState *st_in;      /* [S] the state in front of this push                                       */
    K0DcState *st_out;           /* the same for the next push                                                */
    uint32_t stride, n_blk, R;
};

/* k0_agc_gain: what it reads and leaves for a push of n_blk level blocks per capture */
struct K0AgcArgs {
    const uint8_t *raw;          /* [S][raw_stride] the raw bytes of this push                                */
    uint64_t raw_stride;
    const uint32_t *dc_tab;      /* [S][stride] K0Args.dc_tab (the DC instantiations only)                    */
    uint16_t *tab;               /* [S][stride] K0Args.agc_tab                                                */
    uint32_t stride, n_blk;
};

/* raw bytes per sample; F + 8, the shift behind the gain product */
__host__ __device__ constexpr uint32_t k0_bps(int fmt) { return fmt == WM_K0_CF32 ? 8u : fmt == WM_K0_CS16 ? 4u : 2u; }
__host__ __device__ constexpr uint32_t k0_shift(int fmt, bool sh = false) { return fmt == WM_K0_CS16 || fmt == WM_K0_CF32 ? 30u : sh ? 29u : 23u; }

struct alignas(8) K0U2 { uint32_t x, y; };
struct alignas(16) K0U4 { uint32_t x, y, z, w; };

/* samples of LDS a block needs for its input span: every lane computes WM_K0_OPL outputs, so a partial last group reads
 * (and discards) up to WM_K0_OPL * L outputs past the tile */
__host__ __device__ __forceinline__ uint32_t k0_span(uint32_t L, uint32_t M, uint32_t T, uint32_t tile)
{
    const uint32_t groups = (tile + WM_K0_OPL * L - 1u) / (WM_K0_OPL * L);
    const uint32_t t_max = groups * WM_K0_OPL * L - 1u;
    return (T + 1u + (L - 1u + t_max * M) / L + 1u + 1u) & ~1u;
}
/* a phase's taps in LDS: T / 2 dwords and one of padding -- the lanes of a wave read the same tap pair of up to L different
 * phases at once, and rows T / 2 = 16, 32, ... dwords apart would all start in the same few of the 64 banks */
__host__ __device__ __forceinline__ uint32_t k0_row(uint32_t T) { return T / 2u + 1u; }
/* dynamic LDS of a block, bytes: span dwords | taps | out bytes */
__host__ __device__ __forceinline__ uint32_t k0_lds_bytes(uint32_t L, uint32_t M, uint32_t T, uint32_t tile)
{
    return 4u * k0_span(L, M, T, tile) + 4u * L * k0_row(T) + 2u * tile;
}
/* Outputs per block.  A lane's work item is WM_K0_OPL outputs of one phase, so a tile of WM_K0_OPL * L * g outputs is g * L items:
 * g = floor(512 / L) gives the 256 threads two full trips (481 ... 512 items); fewer where the block's LDS would pass 64 KiB
 * (two blocks and more in a CU's 160 KiB).  0: not even one group fits. */
__host__ __device__ __forceinline__ uint32_t k0_pick_tile(uint32_t L, uint32_t M, uint32_t T)
{
    uint32_t g = 2u * WM_K0_THREADS / L;
    while (g > 1u && k0_lds_bytes(L, M, T, WM_K0_OPL * L * g) > 65536u) g--;
    return k0_lds_bytes(L, M, T, WM_K0_OPL * L * g) > 65536u ? 0u : WM_K0_OPL * L * g;
}

__device__ __forceinline__ uint32_t k0_pack(uint32_t byte_pair)        /* cu8 {I, Q} -> {2I - 255, 2Q - 255} as two int16 */
{
    const int32_t i = 2 * (int32_t)(byte_pair & 0xFFu) - 255, q = 2 * (int32_t)((byte_pair >> 8) & 0xFFu) - 255;
    return ((uint32_t)i & 0xFFFFu) | ((uint32_t)q << 16);
}

/* cf32 -> int16: clamp(rint(f * 32768), -32768, 32767), round half even, NaN -> 0 (the product is exact: a power of two) */
__device__ __forceinline__ int32_t k0_f2x(uint32_t bits)
{
    float f;
    __builtin_memcpy(&f, &bits, 4);
    float v = f * 32768.0f;
    v = v == v ? v : 0.0f;
    return (int32_t)rintf(fminf(fmaxf(v, -32768.0f), 32767.0f));
}
__device__ __forceinline__ uint32_t k0_pair(int32_t i, int32_t q) { return ((uint32_t)i & 0xFFFFu) | ((uint32_t)q << 16); }

/* two consecutive raw samples at p (the first one's index within the push is even: p is aligned to both) -> two LDS dwords */
template <int FMT> __device__ __forceinline__ void k0_load2(const uint8_t *p, uint32_t &v0, uint32_t &v1)
{
    if constexpr (FMT == WM_K0_CS16) {                           /* already the LDS layout */
        const K0U2 w = *(const K0U2 *)p;
        v0 = w.x; v1 = w.y;
    } else if constexpr (FMT == WM_K0_CF32) {
        const K0U4 w = *(const K0U4 *)p;
        v0 = k0_pair(k0_f2x(w.x), k0_f2x(w.y)); v1 = k0_pair(k0_f2x(w.z), k0_f2x(w.w));
    } else {
        uint32_t w = *(const uint32_t *)p;
        if constexpr (FMT == WM_K0_CS8) w ^= 0x80808080u;        /* s + 128: the cu8 byte of the same level */
        v0 = k0_pack(w); v1 = k0_pack(w >> 16);
    }
}
template <int FMT> __device__ __forceinline__ uint32_t k0_load1(const uint8_t *p)
{
    if constexpr (FMT == WM_K0_CS16) return *(const uint32_t *)p;
    else if constexpr (FMT == WM_K0_CF32) { const K0U2 w = *(const K0U2 *)p; return k0_pair(k0_f2x(w.x), k0_f2x(w.y)); }
    else return k0_pack((uint32_t)*(const uint16_t *)p ^ (FMT == WM_K0_CS8 ? 0x8080u : 0u));
}

/* a.lo * b.lo + a.hi * b.hi + c on int16 halves, exact in int32 */
__device__ __forceinline__ int32_t k0_dot2(uint32_t a, uint32_t b, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short k0_s2 __attribute__((ext_vector_type(2)));
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(k0_s2, a), __builtin_bit_cast(k0_s2, b), c, false);
#else
    return c + (int32_t)(int16_t)(a & 0xFFFFu) * (int32_t)(int16_t)(b & 0xFFFFu) + (int32_t)(int16_t)(a >> 16) * (int32_t)(int16_t)(b >> 16);
#endif
}
/* {lo16(s0), lo16(s1)} and {hi16(s0), hi16(s1)} */
__device__ __forceinline__ uint32_t k0_lo_pair(uint32_t s0, uint32_t s1)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(s1, s0, 0x05040100u);
#else
    return (s0 & 0xFFFFu) | (s1 << 16);
#endif
}
__device__ __forceinline__ uint32_t k0_hi_pair(uint32_t s0, uint32_t s1)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(s1, s0, 0x07060302u);
#else
    return (s0 >> 16) | (s1 & 0xFFFF0000u);
#endif
}
/* Frequency shift.  A cu8 / cs8 sample as k0_pack left it, both halves x 64 (|x| <= 16320: the rotation's rounding costs nothing) */
__device__ __forceinline__ uint32_t k0_x64(uint32_t v) { return ((v << 6) & 0x0000FFC0u) | ((v & 0xFFFF0000u) << 6); }
__device__ __forceinline__ int32_t k0_clamp16(int32_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }
/* {xi, xq} times e^(-j phase): the table entry {c, s} of the phase rounded to 10 bits (1024 wraps to 0), {-s, c} from it;
 * yi = (xi c + xq s + 8192) >> 14, yq = (xq c - xi s + 8192) >> 14, each clamped to int16.  |x| (|c| + |s|) < 2^30: exact in int32 */
__device__ __forceinline__ uint32_t k0_rotate(uint32_t x, uint32_t phase, const uint32_t *tab)
{
    const uint32_t cs = tab[(phase + (1u << 21)) >> 22];
    const uint32_t sc = k0_lo_pair(0u - (cs >> 16), cs);
    return k0_pair(k0_clamp16(k0_dot2(x, cs, 8192) >> 14), k0_clamp16(k0_dot2(x, sc, 8192) >> 14));
}
/* I/Q DC blocker: {I - dc_I, Q - dc_Q}, each clamped to int16 (V_PK_SUB_I16 with clamp) */
__device__ __forceinline__ uint32_t k0_sub_dc(uint32_t v, uint32_t dc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef short k0_s2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(k0_s2, v), __builtin_bit_cast(k0_s2, dc)));
#else
    return k0_pair(k0_clamp16((int32_t)(int16_t)(v & 0xFFFFu) - (int32_t)(int16_t)(dc & 0xFFFFu)),
                   k0_clamp16((int32_t)(int16_t)(v >> 16) - (int32_t)(int16_t)(dc >> 16)));
#endif
}
/* the staged sample v (as k0_load2 / k0_load1 left it) of stream index m, rotated; under AFC m is the index within the push and base
 * the phase of the push's first sample (everywhere else the constant 0) */
template <int FMT> __device__ __forceinline__ uint32_t k0_shifted(const K0Args &a, uint32_t v, uint32_t m, uint32_t step, uint32_t base = 0u)
{
    if constexpr (FMT == WM_K0_CU8 || FMT == WM_K0_CS8) v = k0_x64(v);
    return k0_rotate(v, base + step * m, a.shift_tab);
}
/* capture and phase step of pipeline stream v: the stream's own and K0Args.step, or with channels capture v / n_ch and the step of
 * channel v % n_ch (v is blockIdx.y: block-uniform, one scalar division per block), or under AFC what k0_afc_plan left for capture v
 * and this push: {step, base}, and m_first = 0 -- the phase is base + step x (index within the push) instead of step x (index
 * within the stream) */
template <bool SH, bool CH, bool AF = false> __device__ __forceinline__ void k0_capture_of(const K0Args &a, uint32_t v, uint32_t &cp, uint32_t &step, uint32_t &base,
                                                                                          uint32_t &m_first)
{
    cp = v; step = 0u; base = 0u; m_first = (uint32_t)a.in_first;     /* only the low 32 bits of the stream index reach the phase */
    if constexpr (SH) step = a.step;
    if constexpr (CH) { cp = v / a.n_ch; if constexpr (!AF) step = a.steps[v - cp * a.n_ch]; }
    if constexpr (AF) { const K0AfcPush p = a.afc[v]; step = p.step; base = p.base; m_first = 0u; }
}
/* sample k of the four dwords a lane of k0_convert_block loaded, as the {I, Q} int16 pair of the unshifted rules */
template <int FMT> __device__ __forceinline__ uint32_t k0_sample_of(const uint32_t (&in)[4], uint32_t k)
{
    if constexpr (FMT == WM_K0_CS16) return in[k];
    else if constexpr (FMT == WM_K0_CF32) return k0_pair(k0_f2x(in[2u * k]), k0_f2x(in[2u * k + 1u]));
    else return k0_pack(((in[k / 2u] >> (16u * (k & 1u))) & 0xFFFFu) ^ (FMT == WM_K0_CS8 ? 0x8080u : 0u));
}
__device__ __forceinline__ uint32_t k0_byte(int32_t acc)
{
    const int32_t v = (acc + WM_K0_OUT_BIAS) >> 15;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

/* the output stage of every format: g = 256 at F = 15 stays on the 32-bit line above (the branch is uniform); nclip counts the
 * values the clamp changed */
template <int FMT, bool SH = false> __device__ __forceinline__ uint32_t k0_byte_g(int32_t acc, uint32_t g, uint32_t &nclip)
{
    int32_t v;
    if (k0_shift(FMT, SH) == 23u && g == 256u) v = (acc + WM_K0_OUT_BIAS) >> 15;
    else v = (int32_t)(((int64_t)acc * (int64_t)g + ((int64_t)128 << k0_shift(FMT, SH))) >> k0_shift(FMT, SH));
    nclip += (v < 0 || v > 255) ? 1u : 0u;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
/* the same under the per-block AGC: g is the level block's, not the same in every lane, so there is no 32-bit line to stay on */
template <int FMT, bool SH = false> __device__ __forceinline__ uint32_t k0_byte_ag(int32_t acc, uint32_t g, uint32_t &nclip)
{
    const int32_t v = (int32_t)(((int64_t)acc * (int64_t)g + ((int64_t)128 << k0_shift(FMT, SH))) >> k0_shift(FMT, SH));
    nclip += (v < 0 || v > 255) ? 1u : 0u;
    return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
/* U of the AGC rule: g = (96 << U) / P brings a component of size P to 96 (acc g >> (F + 8) is x g / 2^U, with or without a shift) */
__host__ __device__ constexpr uint32_t k0_agc_u(int fmt) { return fmt == WM_K0_CS16 || fmt == WM_K0_CF32 ? 16u : 9u; }
__host__ __device__ __forceinline__ uint32_t k0_agc_rule(uint32_t P, uint32_t U)
{
    const uint32_t g = (WM_K0_AGC_TARGET << U) / (P ? P : 1u);
    return g < 1u ? 1u : g > 65535u ? 65535u : g;
}
__device__ __forceinline__ void k0_add(uint32_t *p, uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;                                                     /* the block emulator runs one lane at a time */
#endif
}
/* a block's clip count -> a.clipped: word is a dword of LDS nobody reads any more; every lane of the block arrives */
__device__ __forceinline__ void k0_count_clips(const K0Args &a, uint32_t *word, uint32_t nclip)
{
    if (!a.clipped) return;
    if (threadIdx.x == 0) *word = 0u;
    __syncthreads();
    if (nclip) k0_add(word, nclip);
    __syncthreads();
    if (threadIdx.x == 0 && *word) k0_add(a.clipped, *word);
}
/* block 0 of a capture: the bytes earlier pushes left go in front of this push's in the window */
__device__ __forceinline__ void k0_carry_rem(const K0Args &a, uint32_t s, uint8_t *out)
{
    const uint16_t *rin = (const uint16_t *)(a.rem_in + (uint64_t)s * 4096u);
    uint16_t *rout = (uint16_t *)(a.rem_out + (uint64_t)s * 4096u);
    for (uint32_t j = threadIdx.x; j < a.rem_prev / 2u; j += blockDim.x) {
        const uint16_t v = rin[j];
        *(uint16_t *)(out + 2u * j) = v;
        if (2u * j >= a.keep_from) rout[(2u * j - a.keep_from) / 2u] = v;
    }
}

/* One block: blockIdx.x = tile, blockIdx.y = capture (with channels: pipeline stream, s; its capture is cp).  lds: k0_lds_bytes()
 * bytes, dword aligned. */
template <int FMT, bool SH = false, bool DC = false, bool AG = false, bool CH = false, bool AF = false> __device__ __forceinline__ void k0_resample_block_t(const K0Args &a, uint32_t *lds)
{
    static_assert(SH || !(CH || AF), "the channels form and the AFC form always rotate");
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, s = blockIdx.y;
    uint32_t cp, step, ph0, m_first;
    k0_capture_of<SH, CH, AF>(a, s, cp, step, ph0, m_first);
    /* the channels form takes the blocker and the AGC as block-uniform runtime branches (K0Args.dc_tab / agc_tab given or not), not as
     * instantiations of their own: DCX / AGX say whether the lines are compiled at all, dc_on / ag_on whether they run.  Without CH they
     * are the constants DC and AG. */
    constexpr bool DCX = DC || CH || AF, AGX = AG || CH || AF;   /* the AFC form takes both as the channels form does */
    const bool dc_on = DC || ((CH || AF) && a.dc_tab != nullptr), ag_on = AG || ((CH || AF) && a.agc_tab != nullptr);
    const uint32_t L = a.L, M = a.M, T = a.T, gain = a.gain_q8 ? a.gain_q8 : 256u;
    constexpr uint32_t BPS = k0_bps(FMT);
    const uint32_t span = k0_span(L, M, T, a.tile);
    uint32_t *xs = lds;                                          /* [span] {I, Q} */
    const uint32_t *tp = lds + span;                             /* [L][k0_row(T)] tap pairs */
    uint16_t *ob = (uint16_t *)(lds + span + L * k0_row(T));     /* [tile] output {I, Q} bytes */
    const uint8_t *raw = a.raw + (uint64_t)cp * a.raw_stride;
    uint8_t *out = a.out + (uint64_t)s * a.out_stride;
    const uint32_t *hist_in = a.hist_in + (uint64_t)s * (T - 1u);

    const uint32_t t_first = blockIdx.x * a.tile;                /* first output of the tile within the push */
    if (t_first >= a.n_out) return;
    const uint32_t ntile = a.n_out - t_first < a.tile ? a.n_out - t_first : a.tile;
    const uint64_t nm = (a.n_first + t_first) * (uint64_t)M;
    const uint64_t q0 = nm / L;                                  /* newest input of the tile's first output, index within the stream */
    const uint32_t r0 = (uint32_t)(nm - q0 * L);                 /* its phase */
    /* LDS sample 0 is input (q0 - (T - 1) - sh) of the stream, sh in {0, 1} so that its index within the push is even */
    const int64_t rel = (int64_t)(q0 - a.in_first) - (int64_t)(T - 1u);     /* within the push; negative: history */
    const uint32_t sh = (uint32_t)(rel & 1);
    const int64_t base = rel - (int64_t)sh;

    for (uint32_t j = 2u * tid; j < span; j += 2u * nthr) {      /* two samples per lane and trip: one aligned load of 4, 8 or 16 bytes of the push */
        const int64_t r = base + (int64_t)j;
        uint32_t v0 = 0u, v1 = 0u;
        if (r >= 0) {
            if (r < (int64_t)a.n_in) {                           /* n_in is even: r + 1 lies inside too */
                k0_load2<FMT>(raw + BPS * (uint64_t)r, v0, v1);
                if constexpr (DCX) if (dc_on) {                  /* r is even: both samples lie in one level block */
                    const uint32_t dc = a.dc_tab[(uint64_t)cp * a.dc_stride + ((uint32_t)r >> WM_K0_DC_LOG2)];
                    v0 = k0_sub_dc(v0, dc); v1 = k0_sub_dc(v1, dc);
                }
                if constexpr (SH) {
                    const uint32_t m = m_first + (uint32_t)r;
                    v0 = k0_shifted<FMT>(a, v0, m, step, ph0); v1 = k0_shifted<FMT>(a, v1, m + 1u, step, ph0);
                }
            }
        } else {                                                 /* r <= -2: both samples are history (the oldest slot, index -T, is never read) */
            const int64_t h = r + (int64_t)(T - 1u);
            if (h >= 0) v0 = hist_in[h];
            if (h + 1 >= 0) v1 = hist_in[h + 1];
        }
        xs[j] = v0; xs[j + 1u] = v1;
    }
    {
        const uint32_t *tg = (const uint32_t *)a.taps;           /* T is a multiple of 16: rows are dword aligned */
        uint32_t *tl = lds + span;
        for (uint32_t j = tid; j < L * T / 2u; j += nthr) tl[j / (T / 2u) * k0_row(T) + j % (T / 2u)] = tg[j];
    }
    if (blockIdx.x == 0) {
        /* the next push's history: the last T - 1 samples of this one (a push is a multiple of 4096 raw bytes, 512 samples of cf32
         * at the least: n_in >= 512 > T - 1) */
        uint32_t *hist_out = a.hist_out + (uint64_t)s * (T - 1u);
        for (uint32_t j = tid; j < T - 1u; j += nthr) {
            const uint32_t r = a.n_in - (T - 1u) + j;
            uint32_t v = k0_load1<FMT>(raw + BPS * (uint64_t)r);
            if constexpr (DCX) if (dc_on) v = k0_sub_dc(v, a.dc_tab[(uint64_t)cp * a.dc_stride + (r >> WM_K0_DC_LOG2)]);
            if constexpr (SH) v = k0_shifted<FMT>(a, v, m_first + r, step, ph0);
            hist_out[j] = v;
        }
        k0_carry_rem(a, s, out);
    }
    __syncthreads();

    const uint32_t groups = (ntile + WM_K0_OPL * L - 1u) / (WM_K0_OPL * L);
    uint32_t nclip = 0u;
    for (uint32_t w = tid; w < groups * L; w += nthr) {
        const uint32_t t0 = (w / L) * WM_K0_OPL * L + w % L;     /* this lane's outputs: t0 + i L */
        const uint32_t v = r0 + t0 * M;
        const uint32_t p = v % L;
        const uint32_t b0 = sh + (T - 1u) + v / L;               /* LDS index of the newest input of output t0; output t0 + i L: + i M */
        const uint32_t *row = tp + p * k0_row(T);
        int32_t ai[WM_K0_OPL], aq[WM_K0_OPL];
#pragma unroll
        for (uint32_t i = 0; i < WM_K0_OPL; i++) { ai[i] = 0; aq[i] = 0; }
        for (uint32_t k = 0; k < T; k += 2u) {
            const uint32_t h2 = row[k / 2u];                     /* {taps[p][k], taps[p][k + 1]} */
#pragma unroll
            for (uint32_t i = 0; i < WM_K0_OPL; i++) {
                const uint32_t s0 = xs[b0 + i * M - k], s1 = xs[b0 + i * M - k - 1u];
                ai[i] = k0_dot2(k0_lo_pair(s0, s1), h2, ai[i]);
                aq[i] = k0_dot2(k0_hi_pair(s0, s1), h2, aq[i]);
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < WM_K0_OPL; i++) {
            const uint32_t t = t0 + i * L;
            if (t >= ntile) continue;
            bool levelled = false;
            if constexpr (AGX) if (ag_on) {                      /* LDS sample j is input base + j of the push; for an output of the push 0 <= that < n_in */
                const uint32_t g = a.agc_tab[(uint64_t)cp * a.dc_stride + ((uint32_t)(base + (int64_t)(b0 + i * M)) >> WM_K0_DC_LOG2)];
                ob[t] = (uint16_t)(k0_byte_ag<FMT, SH>(ai[i], g, nclip) | (k0_byte_ag<FMT, SH>(aq[i], g, nclip) << 8));
                levelled = true;
            }
            if (!levelled) ob[t] = (uint16_t)(k0_byte_g<FMT, SH>(ai[i], gain, nclip) | (k0_byte_g<FMT, SH>(aq[i], gain, nclip) << 8));
        }
    }
    __syncthreads();

    const uint32_t o0 = a.rem_prev + 2u * t_first;               /* window byte of the tile's first output */
    uint16_t *rout = (uint16_t *)(a.rem_out + (uint64_t)s * 4096u);
    for (uint32_t t = tid; t < ntile; t += nthr) {
        const uint16_t v = ob[t];
        const uint32_t o = o0 + 2u * t;
        *(uint16_t *)(out + o) = v;
        if (o >= a.keep_from) rout[(o - a.keep_from) / 2u] = v;
    }
    k0_count_clips(a, xs, nclip);                                /* the span has been read for the last time before the barrier above */
}
__device__ __forceinline__ void k0_resample_block(const K0Args &a, uint32_t *lds) { k0_resample_block_t<WM_K0_CU8>(a, lds); }

/* Conversion only: the input is at decimation x 800 kHz already, output t is input t and acc = 16384 x.  Block = (a.tile consecutive
 * samples, capture); a lane takes 16 raw bytes per load -- 8 / 8 / 4 / 2 samples of cu8 / cs8 / cs16 / cf32 -- and has WM_K0_CONV_UNROLL
 * loads in flight before it converts the first; consecutive lanes load and store consecutive memory.  A push is a multiple of 4096
 * raw bytes, so n_out is a multiple of 512 and rem_prev one of 1024: every store (16, 16, 8, 4 bytes) is aligned to its size and
 * lies on one side of keep_from.  a.tile: a multiple of 8.  word: one dword of LDS for the clip count. */
template <int FMT, bool SH = false, bool DC = false, bool AG = false, bool CH = false, bool AF = false> __device__ __forceinline__ void k0_convert_block(const K0Args &a, uint32_t *word)
{
    static_assert(SH || !(CH || AF), "the channels form and the AFC form always rotate");
    constexpr uint32_t BPS = k0_bps(FMT), SPL = 16u / BPS;       /* samples per lane and load */
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, s = blockIdx.y, gain = a.gain_q8 ? a.gain_q8 : 256u;
    uint32_t cp, step, ph0, m_first;                             /* s: pipeline stream (output, remainder); cp: its capture (raw, level tables) */
    k0_capture_of<SH, CH, AF>(a, s, cp, step, ph0, m_first);
    constexpr bool DCX = DC || CH || AF, AGX = AG || CH || AF;   /* as in k0_resample_block_t: runtime branches in the channels and the AFC form */
    const bool dc_on = DC || ((CH || AF) && a.dc_tab != nullptr), ag_on = AG || ((CH || AF) && a.agc_tab != nullptr);
    const uint8_t *raw = a.raw + (uint64_t)cp * a.raw_stride;
    uint8_t *out = a.out + (uint64_t)s * a.out_stride;
    uint8_t *rout = a.rem_out + (uint64_t)s * 4096u;
    const uint32_t t_first = blockIdx.x * a.tile;
    if (t_first >= a.n_out) return;
    const uint32_t ntile = a.n_out - t_first < a.tile ? a.n_out - t_first : a.tile;
    if (blockIdx.x == 0) k0_carry_rem(a, s, out);
    uint32_t nclip = 0u;
    for (uint32_t i0 = SPL * tid; i0 < ntile; i0 += WM_K0_CONV_UNROLL * SPL * nthr) {
        K0U4 w[WM_K0_CONV_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < WM_K0_CONV_UNROLL; u++) {
            const uint32_t i = i0 + u * SPL * nthr;
            if (i < ntile) w[u] = *(const K0U4 *)(raw + BPS * (uint64_t)(t_first + i));
        }
#pragma unroll
        for (uint32_t u = 0; u < WM_K0_CONV_UNROLL; u++) {
            const uint32_t i = i0 + u * SPL * nthr;
            if (i >= ntile) continue;
            const uint32_t o = a.rem_prev + 2u * (t_first + i);
            uint8_t *dst = o >= a.keep_from ? rout + (o - a.keep_from) : nullptr;
            const uint32_t in[4] = {w[u].x, w[u].y, w[u].z, w[u].w};
            if constexpr (SH || DC || AG) {                      /* every format alike: SPL samples -> SPL byte pairs, one store of 2 SPL bytes */
                const uint32_t m0 = m_first + t_first + i;
                uint32_t r[SPL / 2u];
                uint32_t dc = 0u;                                /* t_first + i is a multiple of SPL: the lane's samples lie in one level block */
                if constexpr (DCX) if (dc_on) dc = a.dc_tab[(uint64_t)cp * a.dc_stride + ((t_first + i) >> WM_K0_DC_LOG2)];
                uint32_t ag = 0u;
                if constexpr (AGX) if (ag_on) ag = a.agc_tab[(uint64_t)cp * a.dc_stride + ((t_first + i) >> WM_K0_DC_LOG2)];
#pragma unroll
                for (uint32_t k = 0; k < SPL; k++) {
                    uint32_t y = k0_sample_of<FMT>(in, k);
                    if constexpr (DCX) if (dc_on) y = k0_sub_dc(y, dc);
                    if constexpr (SH) y = k0_shifted<FMT>(a, y, m0 + k, step, ph0);
                    uint32_t pair;
                    bool levelled = false;
                    if constexpr (AGX) if (ag_on) {
                        pair = k0_byte_ag<FMT, SH>(16384 * (int32_t)(int16_t)(y & 0xFFFFu), ag, nclip) |
                               (k0_byte_ag<FMT, SH>(16384 * (int32_t)(int16_t)(y >> 16), ag, nclip) << 8);
                        levelled = true;
                    }
                    if (!levelled) pair = k0_byte_g<FMT, SH>(16384 * (int32_t)(int16_t)(y & 0xFFFFu), gain, nclip) |
                                (k0_byte_g<FMT, SH>(16384 * (int32_t)(int16_t)(y >> 16), gain, nclip) << 8);
                    r[k / 2u] = k & 1u ? r[k / 2u] | (pair << 16) : pair;
                }
                if constexpr (SPL == 8u) {
                    const K0U4 y = {r[0], r[1], r[2], r[3]};
                    *(K0U4 *)(out + o) = y;
                    if (dst) *(K0U4 *)dst = y;
                } else if constexpr (SPL == 4u) {
                    const K0U2 y = {r[0], r[1]};
                    *(K0U2 *)(out + o) = y;
                    if (dst) *(K0U2 *)dst = y;
                } else {
                    *(uint32_t *)(out + o) = r[0];
                    if (dst) *(uint32_t *)dst = r[0];
                }
            } else if constexpr (FMT == WM_K0_CU8 || FMT == WM_K0_CS8) {
                uint32_t r[4];
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t v = FMT == WM_K0_CS8 ? in[k] ^ 0x80808080u : in[k];
                    r[k] = 0u;
#pragma unroll
                    for (uint32_t b = 0; b < 4u; b++)
                        r[k] |= k0_byte_g<FMT>(16384 * (2 * (int32_t)((v >> (8u * b)) & 0xFFu) - 255), gain, nclip) << (8u * b);
                }
                const K0U4 y = {r[0], r[1], r[2], r[3]};
                *(K0U4 *)(out + o) = y;
                if (dst) *(K0U4 *)dst = y;
            } else if constexpr (FMT == WM_K0_CS16) {
                uint32_t r[2] = {0u, 0u};
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) {
                    r[k / 2u] |= k0_byte_g<FMT>(16384 * (int32_t)(int16_t)(in[k] & 0xFFFFu), gain, nclip) << (16u * (k & 1u));
                    r[k / 2u] |= k0_byte_g<FMT>(16384 * (int32_t)(int16_t)(in[k] >> 16), gain, nclip) << (16u * (k & 1u) + 8u);
                }
                const K0U2 y = {r[0], r[1]};
                *(K0U2 *)(out + o) = y;
                if (dst) *(K0U2 *)dst = y;
            } else {
                uint32_t y = 0u;
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++) y |= k0_byte_g<FMT>(16384 * k0_f2x(in[k]), gain, nclip) << (8u * k);
                *(uint32_t *)(out + o) = y;
                if (dst) *(uint32_t *)dst = y;
            }
        }
    }
    k0_count_clips(a, word, nclip);
}

/* I/Q DC blocker, step 1: S[k] = sum of x over level block k of the push, per I and Q.  blockIdx.x = four level blocks, one per wave;
 * blockIdx.y = capture.  A lane takes 16 raw bytes per load, consecutive lanes consecutive memory: 1 / 1 / 2 / 4 loads cover the 512
 * samples of cu8 / cs8 / cs16 / cf32.  |S| <= 512 * 32768 = 2^24: int32 holds it.  Lanes of a wave leave together or not at all. */
template <int FMT> __device__ __forceinline__ void k0_dc_sums_block(const K0DcArgs &a)
{
    constexpr uint32_t BPS = k0_bps(FMT), SPL = 16u / BPS, LOADS = (BPS << WM_K0_DC_LOG2) / (64u * 16u);
    const uint32_t lane = threadIdx.x & 63u, blk = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u, s = blockIdx.y;
    if (blk >= a.n_blk) return;
    const uint8_t *p = a.raw + (uint64_t)s * a.raw_stride + ((uint64_t)blk << WM_K0_DC_LOG2) * BPS;
    K0U4 w[LOADS];
#pragma unroll
    for (uint32_t j = 0; j < LOADS; j++) w[j] = *(const K0U4 *)(p + 16u * (64u * j + lane));
    int32_t si = 0, sq = 0;
#pragma unroll
    for (uint32_t j = 0; j < LOADS; j++) {
        const uint32_t in[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
        for (uint32_t k = 0; k < SPL; k++) {
            const uint32_t v = k0_sample_of<FMT>(in, k);
            si += (int32_t)(int16_t)(v & 0xFFFFu); sq += (int32_t)(int16_t)(v >> 16);
        }
    }
    uint32_t ui = (uint32_t)si, uq = (uint32_t)sq;               /* wrap-around sums: the order does not matter */
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { ui += __shfl_xor(ui, m); uq += __shfl_xor(uq, m); }
    if (lane == 0) a.sums[(uint64_t)s * a.stride + blk] = K0S2{(int32_t)ui, (int32_t)uq};
}

/* Per-block AGC: g[k] of level block k of the push from its peak P = max(|x'_I| + |x'_Q|), x' behind the blocker where DC is set (the
 * table k0_dc_plan left).  The shape of k0_dc_sums_block: blockIdx.x = four level blocks, one per wave; blockIdx.y = capture; 16 raw
 * bytes per lane and load, all loads of a lane in flight before the first is looked at.  P <= 65536 and maxima do not depend on the
 * order of the reduction.  Lane 0 divides (uint32: 96 << 16 < 2^32) and stores.  Lanes of a wave leave together or not at all. */
template <int FMT, bool DC> __device__ __forceinline__ void k0_agc_gain_block(const K0AgcArgs &a)
{
    constexpr uint32_t BPS = k0_bps(FMT), SPL = 16u / BPS, LOADS = (BPS << WM_K0_DC_LOG2) / (64u * 16u);
    const uint32_t lane = threadIdx.x & 63u, blk = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u, s = blockIdx.y;
    if (blk >= a.n_blk) return;
    const uint8_t *p = a.raw + (uint64_t)s * a.raw_stride + ((uint64_t)blk << WM_K0_DC_LOG2) * BPS;
    K0U4 w[LOADS];
#pragma unroll
    for (uint32_t j = 0; j < LOADS; j++) w[j] = *(const K0U4 *)(p + 16u * (64u * j + lane));
    uint32_t dc = 0u;
    if constexpr (DC) dc = a.dc_tab[(uint64_t)s * a.stride + blk];
    uint32_t peak = 0u;
#pragma unroll
    for (uint32_t j = 0; j < LOADS; j++) {
        const uint32_t in[4] = {w[j].x, w[j].y, w[j].z, w[j].w};
#pragma unroll
        for (uint32_t k = 0; k < SPL; k++) {
            uint32_t v = k0_sample_of<FMT>(in, k);
            if constexpr (DC) v = k0_sub_dc(v, dc);
            const int32_t xi = (int32_t)(int16_t)(v & 0xFFFFu), xq = (int32_t)(int16_t)(v >> 16);
            const uint32_t m = (uint32_t)(xi < 0 ? -xi : xi) + (uint32_t)(xq < 0 ? -xq : xq);
            peak = m > peak ? m : peak;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(peak, m); peak = o > peak ? o : peak; }
    if (lane == 0) a.tab[(uint64_t)s * a.stride + blk] = (uint16_t)k0_agc_rule(peak, k0_agc_u(FMT));
}

/* Lane i's v, the same in every lane of the wave (i is wave-uniform), and the wave's number.  On the device V_READLANE_B32 /
 * V_READFIRSTLANE_B32: what they return lives in scalar registers, so the recurrence below runs on the scalar unit.  On the block
 * emulator the wave meets in a shuffle. */
__device__ __forceinline__ int32_t k0_lane_get(int32_t v, uint32_t i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_readlane(v, (int)i);
#else
    return __shfl(v, (int)i);
#endif
}
__device__ __forceinline__ uint32_t k0_wave_id()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
#else
    return threadIdx.x >> 6;
#endif
}
/* One component (c = 0: I, 1: Q) of one capture: the recurrence over the push's level blocks, in order, by ONE wave.  Its lanes fetch
 * 64 sums at a time; step i takes lane i's sum, moves A -- three scalar instructions in int32, five in int64 -- and puts A[k] into
 * slot i of the wave's 64 slots of LDS (every lane stores the same value: no exec juggling, and the chain never waits for the store);
 * then every lane rounds the A[k] of its own slot to dc[k] and stores it: consecutive lanes, consecutive table entries.  ACC: int32_t
 * where |A| <= 2^(24 + R) fits (R <= 6: the recommended R among them), else int64_t.  |dc| <= 32768 follows from |S| <= 2^24; the
 * clamp is the contract's.  Both waves of the block make the same number of trips: the barrier is uniform. */
template <typename ACC> __device__ __forceinline__ void k0_dc_walk(const K0DcArgs &a, uint32_t s, uint32_t c, uint32_t lane, ACC *slot)
{
    const int32_t *sums = (const int32_t *)(a.sums + (uint64_t)s * a.stride) + c;        /* block k: sums[2 k] */
    int16_t *tab = (int16_t *)(a.tab + (uint64_t)s * a.stride) + c;                       /* block k: tab[2 k] */
    const uint32_t R = a.R;
    ACC acc = (ACC)(c ? a.st_in[s].a_q : a.st_in[s].a_i);
    bool started = a.st_in[s].started != 0u;
    for (uint32_t k0 = 0; k0 < a.n_blk; k0 += 64u) {
        const uint32_t n = a.n_blk - k0 < 64u ? a.n_blk - k0 : 64u;
        const int32_t v = lane < n ? sums[2u * (k0 + lane)] : 0;
        uint32_t i = 0;
        if (!started) {                                          /* A[0] = S[0] << R */
            acc = (ACC)k0_lane_get(v, 0u) * ((ACC)1 << R);
            slot[0] = acc;
            started = true; i = 1u;
        }
        if (i == 0u && n == 64u) {                               /* a whole group: lane numbers and slots are constants */
#pragma unroll
            for (uint32_t j = 0; j < 64u; j += 8u) {             /* eight sums to scalar registers, then eight steps: the chain does not wait for a lane read */
                int32_t sv[8];
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) sv[q] = k0_lane_get(v, j + q);
#if defined(__HIP_DEVICE_COMPILE__)
                __builtin_amdgcn_sched_barrier(0);               /* keep the reads in front: the scheduler would put each back before its use */
#endif
#pragma unroll
                for (uint32_t q = 0; q < 8u; q++) {
                    acc = (ACC)(acc + (ACC)sv[q]) - (acc >> R);  /* >> of a negative value floors */
                    slot[j + q] = acc;
                }
            }
        } else {
            for (; i < n; i++) {
                acc = (ACC)(acc + (ACC)k0_lane_get(v, i)) - (acc >> R);
                slot[i] = acc;
            }
        }
        if (lane < n) tab[2u * (k0 + lane)] = (int16_t)k0_clamp16((int32_t)((slot[lane] + ((ACC)1 << (8u + R))) >> (9u + R)));
        __syncthreads();                                         /* the slots are free again */
    }
    if (lane == 0) {
        if (c) a.st_out[s].a_q = (int64_t)acc; else { a.st_out[s].a_i = (int64_t)acc; a.st_out[s].started = started ? 1u : 0u; }
    }
}
/* step 2: blockIdx.x = capture, two waves: wave 0 walks I, wave 1 walks Q (the recurrence is sequential by definition -- the floor
 * makes it no scan -- so a push's 8192 steps are latency, and the two components at least run side by side).  slots: 128 int64_t */
__device__ __forceinline__ void k0_dc_plan_block(const K0DcArgs &a, int64_t *slots)
{
    const uint32_t lane = threadIdx.x & 63u, c = k0_wave_id(), s = blockIdx.x;
    if (a.R <= 6u) k0_dc_walk<int32_t>(a, s, c, lane, (int32_t *)slots + 64u * c); else k0_dc_walk<int64_t>(a, s, c, lane, slots + 64u * c);
}

#if defined(__HIPCC__)
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_dc_sums(K0DcArgs a) { k0_dc_sums_block<FMT>(a); }
__global__ void __launch_bounds__(128) k0_dc_plan(K0DcArgs a)
{
    __shared__ int64_t slots[128];
    k0_dc_plan_block(a, slots);
}
/* cfg.input_dc: the two stages with the subtraction in their staging, with and without the rotation */
template <int FMT, bool SH> __global__ void __launch_bounds__(WM_K0_THREADS) k0_resample_dc(K0Args a)
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block_t<FMT, SH, true>(a, k0_lds);
}
template <int FMT, bool SH> __global__ void __launch_bounds__(WM_K0_THREADS) k0_convert_dc(K0Args a)
{
    __shared__ uint32_t word;
    k0_convert_block<FMT, SH, true>(a, &word);
}
/* cfg.input_agc: the gain kernel, and the two stages with the level block's gain in their output stage */
template <int FMT, bool DC> __global__ void __launch_bounds__(WM_K0_THREADS) k0_agc_gain(K0AgcArgs a) { k0_agc_gain_block<FMT, DC>(a); }
template <int FMT, bool SH, bool DC> __global__ void __launch_bounds__(WM_K0_THREADS) k0_resample_agc(K0Args a)
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block_t<FMT, SH, DC, true>(a, k0_lds);
}
template <int FMT, bool SH, bool DC> __global__ void __launch_bounds__(WM_K0_THREADS) k0_convert_agc(K0Args a)
{
    __shared__ uint32_t word;
    k0_convert_block<FMT, SH, DC, true>(a, &word);
}
/* cfg.input_channels: the two stages with a capture per n_ch pipeline streams and a phase step per channel; the rotation is always on,
 * the blocker and the AGC are runtime branches on K0Args.dc_tab / agc_tab (one instantiation per format: DC x AG as template parameters
 * were 32 more kernels and a third more compile time for the whole library) */
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_resample_ch(K0Args a)
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block_t<FMT, true, false, false, true>(a, k0_lds);
}
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_convert_ch(K0Args a)
{
    __shared__ uint32_t word;
    k0_convert_block<FMT, true, false, false, true>(a, &word);
}
/* cfg.input_afc: the two stages with a {step, base} per capture and push from k0_afc_plan (wm_k0_afc.h) and a push-local sample index;
 * the rotation is always on, the blocker and the AGC are runtime branches, as in the channels form and for the same reason */
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_resample_afc(K0Args a)
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block_t<FMT, true, false, false, false, true>(a, k0_lds);
}
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_convert_afc(K0Args a)
{
    __shared__ uint32_t word;
    k0_convert_block<FMT, true, false, false, false, true>(a, &word);
}
/* cfg.input_channel_afc_hz: the channels form with a {step, base} per pipeline stream and push from k0_afc_plan */
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_resample_ch_afc(K0Args a)
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block_t<FMT, true, false, false, true, true>(a, k0_lds);
}
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_convert_ch_afc(K0Args a)
{
    __shared__ uint32_t word;
    k0_convert_block<FMT, true, false, false, true, true>(a, &word);
}
__global__ void __launch_bounds__(WM_K0_THREADS) k0_resample(K0Args a)          /* cu8 */
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block(a, k0_lds);
}
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_resample_fmt(K0Args a)
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block_t<FMT>(a, k0_lds);
}
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_convert(K0Args a)
{
    __shared__ uint32_t word;
    k0_convert_block<FMT>(a, &word);
}
/* cfg.input_shift_hz: the same two stages with the rotation in their staging */
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_resample_shift(K0Args a)
{
    extern __shared__ uint32_t k0_lds[];
    k0_resample_block_t<FMT, true>(a, k0_lds);
}
template <int FMT> __global__ void __launch_bounds__(WM_K0_THREADS) k0_convert_shift(K0Args a)
{
    __shared__ uint32_t word;
    k0_convert_block<FMT, true>(a, &word);
}
#endif

#endif
