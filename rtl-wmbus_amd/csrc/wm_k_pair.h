/* wm_k_pair.h -- the latency-bound framer and burst kernels as PAIRED launches: one launch with gridDim.z = 2 carries the
 * blocks of two receiver contexts (a batch lane, wm_batch.h).  Both argument sets travel in the kernarg segment; a block
 * picks its own by blockIdx.z (uniform: scalar loads at an offset) and runs the very block function of the plain kernel with
 * its own context's grid extent -- the launch's grid is the larger of the two, a block outside its context's extent
 * returns at once.  The plain kernels are untouched: a context outside a lane, and a lane's operation whose mate has no
 * equal one, launches those. */
#ifndef WM_K_PAIR_H
#define WM_K_PAIR_H

template <typename A> struct WmPair {
    A a[2];
    uint32_t gx[2], gy[2];       /* every context's own grid */
};

struct K3ScanArgs {
    WmPush g;
    const uint32_t *chips0, *chips1, *counts0, *counts1, *seen0, *seen1;
    uint2 *hits; uint32_t *n_hits; uint32_t hits_cap; uint32_t *err;
};
struct K3SpansArgs { K3Args a; uint32_t tile_len, ntiles; uint32_t *flags, *list, *n_list; };
struct K3BurstsArgs { K3Args a; uint32_t n_items_host; };

#ifdef __HIPCC__

#define WM_PAIR_MINE(p, z) const uint32_t z = blockIdx.z; if (blockIdx.x >= (p).gx[z] || blockIdx.y >= (p).gy[z]) return

__global__ __launch_bounds__(64 * WM_RLA_WPB, WM_RLA_WAVES_PER_SIMD) void k2_rla_pair(WmPair<K2Args> p)
{
    wm_framer_prio();
    WM_PAIR_MINE(p, z);
    __shared__ RlaLds lds;
    rla_lds_init(lds, threadIdx.x, 64 * WM_RLA_WPB);
    __syncthreads();
    rla_lanes<0>(p.a[z], blockIdx.x, lds);
}

__global__ __launch_bounds__(64 * WM_RLA_WPB, WM_RLA_WAVES_PER_SIMD) void k2_rla_list_pair(WmPair<K2Args> p)
{
    wm_framer_prio();
    WM_PAIR_MINE(p, z);
    __shared__ RlaLds lds;
    rla_lds_init(lds, threadIdx.x, 64 * WM_RLA_WPB);
    __syncthreads();
    const K2Args &a = p.a[z];
    const uint32_t n = k2_lane_count(a);
    for (uint32_t b = blockIdx.x; (uint64_t)b * (64u * WM_RLA_WPB) < n; b += p.gx[z]) rla_lanes<1>(a, b, lds);
}

template <bool DC, bool COOP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k2_clock_sys_pair(WmPair<K2Args> p)
{
    wm_framer_prio();
    WM_PAIR_MINE(p, z);
    clock_sys_group<DC, 0, COOP>(p.a[z], blockIdx.x, *(ClkSysLds *)wm_sys_lds);
}

template <bool DC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k2_clock_sys_list_pair(WmPair<K2Args> p)
{
    wm_framer_prio();
    WM_PAIR_MINE(p, z);
    const K2Args &a = p.a[z];
    const uint32_t n = k2_lane_count(a);
    for (uint32_t b = blockIdx.x; (uint64_t)b * 64u < n; b += p.gx[z]) clock_sys_group<DC, 1, false>(a, b, *(ClkSysLds *)wm_sys_lds);
}

__global__ __launch_bounds__(256) void k3_scan_pair(WmPair<K3ScanArgs> p)
{
    wm_framer_prio();
    WM_PAIR_MINE(p, z);
    const K3ScanArgs &a = p.a[z];
    k3_scan_block(a.g, a.chips0, a.chips1, a.counts0, a.counts1, a.seen0, a.seen1, a.hits, a.n_hits, a.hits_cap, a.err, blockIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void k3_spans_pair(WmPair<K3SpansArgs> p)
{
    wm_framer_prio();
    WM_PAIR_MINE(p, z);
    const K3SpansArgs &a = p.a[z];
    k3_spans_block(a.a, a.tile_len, a.ntiles, a.flags, a.list, a.n_list, blockIdx.x, p.gx[z]);
}

__global__ __launch_bounds__(256) void k3_bursts_pair(WmPair<K3BurstsArgs> p)
{
    wm_framer_prio();
    WM_PAIR_MINE(p, z);
    __shared__ K3Lds lds;
    const K3BurstsArgs &a = p.a[z];
    k3_bursts_block(a.a, a.n_items_host, lds, blockIdx.x, p.gx[z]);
}

#endif /* __HIPCC__ */

#endif /* WM_K_PAIR_H */
