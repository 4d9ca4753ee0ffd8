/* wm_launch.h -- the one layer through which the two halves of a push (enqueue_front_impl, enqueue_back_impl and their
 * helpers) put work on a context's stream.  Part of wm_api.hip's translation unit (inside its unnamed namespace).
 *
 * Outside a batch lane every call issues its operation at once, exactly as the call it replaces did.  A lane (wm_batch.h)
 * sets wmbus_ctx.rec: the operation is appended to that list instead, with its arguments as they are NOW (by value; only
 * the stream is looked up when the operation leaves -- a lane's contexts run on the lane's stream).  The lane records the
 * same half of both its contexts, merges the two lists (wm_lane_merge.h) and issues them: two equal pairable kernels as
 * one launch with gridDim.z = 2 (wm_k_pair.h), everything else singly in its context's own order. */
#ifndef WM_LAUNCH_H
#define WM_LAUNCH_H

struct WmLaneOp {
    WmLaneKey key{0u, 0u, 0u};
    const char *what = "";
    bool launch = false;                                   /* a kernel launch (counted by wmbus_batch_lane_stats) */
    std::function<hipError_t()> run;                       /* the operation on its own */
    dim3 grid;                                             /* pairable launches: this context's grid ... */
    std::shared_ptr<void> args;                            /* ... its argument struct ... */
    hipError_t (*pair)(hipStream_t, const WmLaneOp &, const WmLaneOp &) = nullptr;      /* ... and the launch of two of them as one */
};
struct WmLaneRec { std::vector<WmLaneOp> ops; };

/* any operation: `f` is called now, or when the lane issues it */
template <typename F> int wm_op(wmbus_ctx *c, const char *what, F f, bool launch = false)
{
    if (c->rec) {
        WmLaneOp op;
        op.what = what; op.launch = launch; op.run = std::move(f);
        c->rec->ops.push_back(std::move(op));
        return 0;
    }
    const hipError_t e = f();
    return e == hipSuccess ? 0 : fail(c, WMBUS_EDEVICE, "%s: %s", what, hipGetErrorString(e));
}

/* a kernel launch on the context's stream (errors surface at the next hipGetLastError, as before) */
template <typename... KA, typename... A> void wm_launch(wmbus_ctx *c, void (*k)(KA...), dim3 grid, dim3 block, uint32_t lds, A... args)
{
    if (!c->rec) { c->n_single++; hipLaunchKernelGGL(k, grid, block, lds, c->stream, args...); return; }
    wm_op(c, "kernel launch", [=] { hipLaunchKernelGGL(k, grid, block, lds, c->stream, args...); return hipGetLastError(); }, true);
}

/* a launch of a kernel that has a paired form `kp`: `single(stream)` launches the plain kernel as before, `a` is the whole
 * argument list as the paired form takes it */
template <typename A, typename Single> void wm_launch_pairable(wmbus_ctx *c, Single single, void (*kp)(WmPair<A>), dim3 grid, uint32_t block, uint32_t lds, const A &a)
{
    if (!c->rec) { c->n_single++; single(c->stream); return; }
    WmLaneOp op;
    op.key = WmLaneKey{(uint64_t)(uintptr_t)kp, block, lds};
    op.what = "kernel launch"; op.launch = true; op.grid = grid;
    op.args = std::make_shared<A>(a);
    op.run = [=] { single(c->stream); return hipGetLastError(); };
    op.pair = [](hipStream_t st, const WmLaneOp &x, const WmLaneOp &y) {
        WmPair<A> p;
        p.a[0] = *(const A *)x.args.get(); p.a[1] = *(const A *)y.args.get();
        p.gx[0] = x.grid.x; p.gx[1] = y.grid.x; p.gy[0] = x.grid.y; p.gy[1] = y.grid.y;
        void (*const pk)(WmPair<A>) = (void (*)(WmPair<A>))(uintptr_t)x.key.kind;
        hipLaunchKernelGGL(pk, dim3(std::max(x.grid.x, y.grid.x), std::max(x.grid.y, y.grid.y), 2u), dim3(x.key.block), x.key.lds, st, p);
        return hipGetLastError();
    };
    c->rec->ops.push_back(std::move(op));
}

/* the other stream operations of a push, on the context's stream */
#define WM_OP(c, what, ...) do { const int rc_ = wm_op((c), what, __VA_ARGS__); if (rc_) return rc_; } while (0)
#define wm_memset(c, p, v, n) do { void *const p_ = (void *)(p); const int v_ = (v); const size_t n_ = (n); wmbus_ctx *const c_ = (c); \
    WM_OP(c_, "hipMemsetAsync", [=] { return hipMemsetAsync(p_, v_, n_, c_->stream); }); } while (0)
#define wm_memcpy(c, dst, src, n, kind) do { void *const d_ = (void *)(dst); const void *const s_ = (const void *)(src); const size_t n_ = (n); wmbus_ctx *const c_ = (c); \
    WM_OP(c_, "hipMemcpyAsync", [=] { return hipMemcpyAsync(d_, s_, n_, (kind), c_->stream); }); } while (0)
#define wm_record(c, event) do { const hipEvent_t e_ = (event); wmbus_ctx *const c_ = (c); \
    WM_OP(c_, "hipEventRecord", [=] { return hipEventRecord(e_, c_->stream); }); } while (0)
#define wm_wait(c, event) do { const hipEvent_t e_ = (event); wmbus_ctx *const c_ = (c); \
    WM_OP(c_, "hipStreamWaitEvent", [=] { return hipStreamWaitEvent(c_->stream, e_, 0); }); } while (0)

#endif /* WM_LAUNCH_H */
