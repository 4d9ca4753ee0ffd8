/* wm_resample_design.h -- host side of K0 (wm_k0_resample.h): the polyphase taps, designed in double by the library.
 * Part of wm_api.hip's translation unit; needs no device.
 *
 * L / M = out_hz / in_hz reduced.  Prototype: Kaiser-windowed sinc (beta 8) of N = L T taps at the rate L in_hz, cut-off
 * 0.45 min(in_hz, out_hz), T = 16 max(1, ceil(M / L)).  Phase p owns prototype taps p, p + L, p + 2L, ...; every phase is scaled
 * to sum 1, multiplied by 16384 and rounded to int16; what the rounded phase then misses of 16384 is spread one LSB per tap over
 * the taps with the largest rounding remainders, so that EVERY phase sums to exactly 16384: no phase-dependent gain, the half-LSB
 * offset of the output stays exact, and every tap is within one LSB of its value.  (Putting the whole rest on the phase's largest
 * tap, as an earlier version did, costs up to 6 dB of stop band at T = 512, where a phase misses its sum by 6 LSB rms:
 * tests/test_resampler_design.py::test_response_against_the_float_design.) */
#ifndef WM_RESAMPLE_DESIGN_H
#define WM_RESAMPLE_DESIGN_H

namespace {

double k0_bessel_i0(double x)
{
    double sum = 1., term = 1.;
    const double q = x * x / 4.;
    for (int k = 1; k < 200; k++) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}

/* 0, or a message for WMBUS_EINVAL.  taps may be NULL (geometry only). */
const char *k0_design(unsigned in_hz, unsigned out_hz, unsigned *pL, unsigned *pM, unsigned *pT, int16_t *taps, size_t cap)
{
    if (in_hz < 800000u) return "input_rate_hz must be at least 800000";
    if (out_hz == 0u || out_hz % 800000u) return "the output rate must be a multiple of 800000";
    const unsigned g = std::gcd(in_hz, out_hz);
    const unsigned L = out_hz / g, M = in_hz / g;
    if (L > WM_K0_MAX_L || M > WM_K0_MAX_M) return "input_rate_hz: output rate / input rate = L / M in lowest terms needs L <= 32 and M <= 1024";
    const unsigned T = 16u * std::max(1u, (M + L - 1u) / L);
    if (T > WM_K0_MAX_T) return "input_rate_hz: more than 32 input samples per output sample";
    if (pL) *pL = L;
    if (pM) *pM = M;
    if (pT) *pT = T;
    if (!taps) return nullptr;
    if (cap < (size_t)L * T) return "resampler design: tap buffer too small";
    const size_t N = (size_t)L * T;
    std::vector<double> h(N);
    const double fc = 0.45 * (double)std::min(in_hz, out_hz), fs = (double)L * (double)in_hz, mid = ((double)N - 1.) / 2.;
    const double i0b = k0_bessel_i0(8.);
    for (size_t i = 0; i < (N + 1) / 2; i++) {                  /* one half computed, the other mirrored: exactly symmetric */
        const double t = (double)i - mid, a = 2. * fc / fs * t;
        const double sinc = a == 0. ? 1. : sin(M_PI * a) / (M_PI * a);
        const double r = t / mid;
        h[i] = h[N - 1 - i] = sinc * k0_bessel_i0(8. * sqrt(std::max(0., 1. - r * r))) / i0b;
    }
    for (unsigned p = 0; p < L; p++) {
        /* phases p and L - 1 - p are mirror images: one sum serves both, so that they round alike */
        const unsigned pa = std::min(p, L - 1u - p);
        double sum = 0.;
        for (unsigned k = 0; k < T; k++) sum += h[pa + (size_t)L * k];
        long total = 0, abs_total = 0;
        std::vector<std::pair<double, unsigned>> rest(T);       /* (what rounding took from tap k, towards the correction; k) */
        for (unsigned k = 0; k < T; k++) {
            const double x = h[p + (size_t)L * k] / sum * 16384.;
            const long v = lround(x);
            taps[(size_t)p * T + k] = (int16_t)v;
            total += v;
            rest[k] = {x - (double)v, k};
        }
        /* the phase must sum to 16384: the |16384 - total| taps that rounding moved furthest the other way take one LSB each (largest
         * remainders first), so no tap ends a whole LSB from its value.  Equal remainders go by index, counted from the other end in
         * the mirrored phase: the prototype stays symmetric. */
        const long miss = 16384 - total, step = miss < 0 ? -1 : 1;
        const bool mirrored = p > L - 1u - p;
        if (labs(miss) > (long)T) return "resampler design: a phase is more than one LSB per tap from its sum";
        std::sort(rest.begin(), rest.end(), [&](const std::pair<double, unsigned> &a, const std::pair<double, unsigned> &b) {
            const double ka = a.first * (double)step, kb = b.first * (double)step;
            if (ka != kb) return ka > kb;
            return mirrored ? a.second > b.second : a.second < b.second;
        });
        for (long i = 0; i < labs(miss); i++) {
            const long fixed = (long)taps[(size_t)p * T + rest[(size_t)i].second] + step;
            if (fixed > 32767 || fixed < -32768) return "resampler design: a tap leaves int16";
            taps[(size_t)p * T + rest[(size_t)i].second] = (int16_t)fixed;
        }
        for (unsigned k = 0; k < T; k++) abs_total += labs((long)taps[(size_t)p * T + k]);
        /* |acc| <= 255 sum|taps|: far inside int32 (the kernel's accumulator) and, with the output bias, inside 2^31 */
        if (255l * abs_total + WM_K0_OUT_BIAS >= (1l << 30)) return "resampler design: accumulator bound exceeded";
    }
    return nullptr;
}

/* The frequency shift of cfg.input_shift_hz (the arithmetic is in include/wmbus_hip.h): the phase step per input sample as a
 * fraction of 2^32, rounded to nearest with floor division (also for a negative shift), and the 1024-entry table {c, s} =
 * rint(16384 cos / sin(2 pi i / 1024)) in double.  0, or a message for WMBUS_EINVAL.  table may be NULL (the step only). */
#define WM_K0_SHIFT_ENTRIES 1024u
const char *k0_shift_design(unsigned in_hz, int shift_hz, uint32_t *step, int16_t *table, size_t cap)
{
    if (in_hz < 800000u) return "the input rate must be at least 800000";
    const int64_t f = shift_hz, fin = in_hz;
    if (2 * (f < 0 ? -f : f) > fin) return "input_shift_hz must lie within +- half the input rate";
    const int64_t num = f * ((int64_t)1 << 32) + fin / 2;       /* |f| <= 2^31 - 1: inside int64 */
    int64_t q = num / fin;
    if (num % fin < 0) q--;                                      /* floor, not C's truncation */
    if (step) *step = (uint32_t)(uint64_t)q;
    if (!table) return nullptr;
    if (cap < 2u * WM_K0_SHIFT_ENTRIES) return "shift design: table buffer too small";
    for (unsigned i = 0; i < WM_K0_SHIFT_ENTRIES; i++) {
        const double w = 2. * M_PI * (double)i / (double)WM_K0_SHIFT_ENTRIES;
        table[2u * i] = (int16_t)rint(16384. * cos(w));
        table[2u * i + 1u] = (int16_t)rint(16384. * sin(w));
    }
    return nullptr;
}

}  // namespace
#endif
