/* wm_spectrum_channels.h -- host side of the channel survey (wm_k0_spectrum.h): the rule that turns the two arrays of
 * wmbus_read_spectrum into a list of channels.  Part of wm_api.hip's translation unit; needs no device.  The rule is written out in
 * include/wmbus_hip.h (SPECTRUM) and restated in Python integers in tests/spectrum_ref.py; the intermediate arithmetic is 128 bits wide
 * (2 num in_hz reaches 2^81). */
#ifndef WM_SPECTRUM_CHANNELS_H
#define WM_SPECTRUM_CHANNELS_H

namespace {

typedef __int128 k0_i128;

k0_i128 k0_floor_div(k0_i128 a, k0_i128 b)                      /* b > 0; floors also for a < 0 */
{
    k0_i128 q = a / b;
    if (a % b < 0) q--;
    return q;
}

int k0_spectrum_channels(unsigned in_hz, const uint64_t *sum, const uint32_t *peak, uint64_t blocks, unsigned width_hz, unsigned min_ratio_q8,
                         unsigned rel, wmbus_channel_hit *out, unsigned cap)
{
    constexpr int N = 512;
    if (!width_hz) width_hz = 200000u;
    if (!min_ratio_q8) min_ratio_q8 = 1024u;
    if (!rel) rel = 8u;
    if (!sum || !peak || (!out && cap) || in_hz < 800000u || blocks == 0u || min_ratio_q8 < 257u) return WMBUS_EINVAL;
    const int W = (int)std::min<uint64_t>(std::max<uint64_t>((uint64_t)width_hz * N / in_hz, 1u), 256u);
    std::vector<uint32_t> sp(peak, peak + N);
    std::vector<uint64_t> sm(N);
    for (int b = 0; b < N; b++) sm[b] = sum[b] / blocks;
    std::nth_element(sp.begin(), sp.begin() + 255, sp.end());
    std::nth_element(sm.begin(), sm.begin() + 255, sm.end());
    const uint32_t Fp = std::max<uint32_t>(1u, sp[255]);
    const uint32_t Fm = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1u, sm[255]), 0xFFFFFFFFu);
    const int nB = N - W + 1;
    std::vector<uint64_t> B(nB);
    std::vector<char> alive(nB, 1);
    uint64_t run = 0;
    for (int i = 0; i < W; i++) run += peak[i];
    for (int b = 0; b < nB; b++) { B[b] = run; if (b + W < N) run += (uint64_t)peak[b + W] - peak[b]; }
    unsigned hits = 0;
    uint64_t first = 0;
    while (hits < cap) {
        int best = -1;
        for (int b = 0; b < nB; b++) if (alive[b] && (best < 0 || B[b] > B[best])) best = b;
        if (best < 0 || (k0_i128)B[best] * 256 < (k0_i128)min_ratio_q8 * W * Fp || (hits && (k0_i128)B[best] * rel < (k0_i128)first)) break;
        if (!hits) first = B[best];
        int lo = best;
        k0_i128 num = 0, den = 0;
        for (int trip = 0; trip < 3; trip++) {
            k0_i128 d = 0, n = 0;
            for (int i = lo; i < lo + W; i++) {
                const int64_t e = peak[i] > Fp ? (int64_t)(peak[i] - Fp) : 0;
                d += e; n += (k0_i128)e * (i - 256);
            }
            if (d == 0) break;                                   /* never on the first trip (min_ratio_q8 > 256); later: the last window stands */
            den = d; num = n;
            const int64_t cb = (int64_t)k0_floor_div(2 * num + den, 2 * den);
            const int nlo = (int)std::min<int64_t>(std::max<int64_t>(cb + 256 - W / 2, 0), N - W);
            if (nlo == lo) break;
            lo = nlo;
        }
        wmbus_channel_hit &h = out[hits++];
        h.offset_hz = (int32_t)k0_floor_div(2 * num * in_hz + (k0_i128)N * den, (k0_i128)2 * N * den);
        const k0_i128 ratio = (k0_i128)B[best] * 256 / ((k0_i128)W * Fp);
        h.ratio_q8 = ratio > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)ratio;
        h.floor_peak = Fp; h.floor_mean = Fm;
        for (int b = std::max(0, best - W + 1); b < std::min(nB, best + W); b++) alive[b] = 0;
    }
    return (int)hits;
}

}  // namespace
#endif
