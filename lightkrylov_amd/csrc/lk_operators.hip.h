// lk_operators.hip.h -- the operators of the C ABI: one type per kind behind lk_linop_s, their creators and lk_linop_apply.
// Part of lk_engine.hip's translation unit (the kernels are compiled once): included inside its extern "C" block, after the helpers
// used here -- ProfScope, launch_profiled, DevGuard, allreduce, blas1_grid, lazy_enter_vec, check_vec, check_pair.
#pragma once

extern "C++" {   // the include sits inside the engine's extern "C" block, and a template cannot have C linkage
// What every kind is to the rest of the engine.  `apply` ENQUEUES y = op(A) x on the context's stream for this rank's rows; the checks
// and the bookkeeping on the two vectors are lk_linop_apply's.
struct lk_linop_s {
    lk_context_t ctx;
    int dtype;
    int64_t n;                                                       // rows (= entries of x and y) held by this rank
    // the "matvec" profiling scope: algorithmic bytes of one product (0 = not priced), and whether the product is ONE kernel that
    // carries the scope's two events on its own dispatch, like the sweeps: no marker packets
    double matvec_bytes = 0.0;
    bool one_kernel = false;
    lk_linop_s(lk_context_t c, int dt, int64_t rows) : ctx(c), dtype(dt), n(rows) {}
    virtual ~lk_linop_s() = default;                                 // what a kind owns goes with it (the frees synchronise); ctx is not touched
    virtual int apply(int trans, const double *x, double *y, ProfScope &ps) = 0;
    // the row-local form of the operator for the Gram-Schmidt sweeps (fused_rowop); kind ROWOP_NONE: there is none
    virtual RowOp rowop(int trans, int basis_dtype) const { (void)trans; (void)basis_dtype; return RowOp{}; }
    int ed() const { return dtype == LK_C128 ? 2 : 1; }
};

namespace {
// the single kernel (256 threads per block) of an operator with `one_kernel` set: the extended launch when the scope wants its events on the dispatch
template <class... A, class... B>
int launch_in_scope(ProfScope &ps, void (*kern)(A...), int grid, const B &...args) {
    launch_profiled(ps, kern, dim3(grid), dim3(256), 0, ps.c->stream, args...);
    return LK_OK;
}

// ---- diagonal: y = D x, D given entry by entry ----------------------------------------------------------------------------------
struct DiagOp final : lk_linop_s {
    DevBuf<double> d;
    DiagOp(lk_context_t c, int dt, int64_t rows) : lk_linop_s(c, dt, rows) { matvec_bytes = 3.0 * n * ed() * 8.0; one_kernel = true; }   // d, x read, y written
    int apply(int trans, const double *x, double *y, ProfScope &ps) override {
        const bool cp = dtype == LK_C128;
        return launch_in_scope(ps, cp ? k_diag<true> : k_diag<false>, blas1_grid(ctx, n * ed() / 2 + 1), d, x, y, n, (int)(cp && trans == LK_OP_H), ctx->guard());
    }
    RowOp rowop(int trans, int basis_dtype) const override { return RowOp{ROWOP_DIAG, trans && basis_dtype == LK_C128, 0.0, 0.0, 0, d}; }
};

// ---- generated diagonal: d_i = d0 + dstep (row0 + i), real kind -----------------------------------------------------------------
struct DiagLinOp final : lk_linop_s {
    int64_t row0 = 0;
    double d0 = 0, dstep = 0;
    DiagLinOp(lk_context_t c, int64_t rows) : lk_linop_s(c, LK_F64, rows) { matvec_bytes = 2.0 * n * 8.0; one_kernel = true; }          // x read, y written
    int apply(int, const double *x, double *y, ProfScope &ps) override {
        return launch_in_scope(ps, k_diag_linspace, blas1_grid(ctx, n / 2 + 1), d0, dstep, row0, x, y, n, ctx->guard());
    }
    RowOp rowop(int, int basis_dtype) const override { return basis_dtype == LK_F64 ? RowOp{ROWOP_LIN, 0, d0, dstep, row0, nullptr} : RowOp{}; }
};

// ---- the row partition of a sharded matrix (dense, CSR) -------------------------------------------------------------------------
// This rank holds rows [row0, row0 + n) of an ncols_g x ncols_g operator.  'N' multiplies them with the all-gathered x; 'H' applies
// their conjugate transpose to this rank's x: full-length partial sums, summed over the ranks, of which this rank keeps its rows.
struct RowPartition {
    int64_t ncols_g = 0;                     // global size (= n on a single rank)
    int64_t row0 = 0;
    std::vector<int64_t> gcounts, gdispls;   // all-gather layout in DOUBLES (per rank)
    DevBuf<double> xfull;                    // the gathered input vector / the full-length adjoint product (ncols_g elements)
    // layout of the all-gather of x (counts and displacements in doubles) + the workspace; *n_local = rows of this rank
    int shard_setup(lk_context_t c, int ED, int64_t n_global, const int64_t *row_starts, const char *what, int64_t *n_local) {
        if (!row_starts) return fail(LK_ERR_INVALID, "%s: null row_starts", what);
        if (row_starts[0] != 0 || row_starts[c->nranks] != n_global) return fail(LK_ERR_INVALID, "%s: row_starts must run from 0 to n_global", what);
        for (int r = 0; r < c->nranks; ++r)
            if (row_starts[r + 1] < row_starts[r]) return fail(LK_ERR_INVALID, "%s: row_starts decreases at rank %d", what, r);
        ncols_g = n_global;
        *n_local = row_starts[c->rank + 1] - row_starts[c->rank];
        row0 = row_starts[c->rank];
        gcounts.resize(c->nranks); gdispls.resize(c->nranks);
        for (int r = 0; r < c->nranks; ++r) {
            gcounts[r] = (row_starts[r + 1] - row_starts[r]) * ED;
            gdispls[r] = row_starts[r] * ED;
        }
        if (c->nranks > 1) LKCHK(xfull.reserve((n_global > 0 ? n_global : 1) * ED));
        return LK_OK;
    }
    // x (this rank's rows) -> the full-length buffer, rank r's block at its global offset; one rank: x itself
    int gather_x(lk_context_t c, int ED, const double *x, const double **xg) {
        if (c->nranks == 1) { *xg = x; return LK_OK; }
        if (!c->allgather) return fail(LK_ERR_COMM, "row-sharded dense / CSR operator but no all-gather installed (lk_comm_init_rank / lk_set_allgather)");
        ProfScope ps(c, "comm_allgather", (double)ncols_g * (ED == 2 ? 16.0 : 8.0));
        const int rc = c->allgather(c->allgather_user, x, xfull, gcounts.data(), gdispls.data(), c->nranks, (void *)c->stream);
        if (rc != 0) return fail(LK_ERR_COMM, "all-gather callback returned %d", rc);
        *xg = xfull;
        return LK_OK;
    }
    // where the 'H' product of this rank's row block is written: y itself on one rank, the full-length buffer otherwise ...
    double *adjoint_out(lk_context_t c, double *y) const { return c->nranks > 1 ? (double *)xfull : y; }
    // ... which is then summed over the ranks; this rank keeps its n rows in y
    int reduce_to_slice(lk_context_t c, int ED, int64_t n, double *y) {
        if (c->nranks == 1) return LK_OK;
        LKCHK(allreduce(c, xfull, ncols_g * ED));
        const int64_t nd = n * ED;
        hipLaunchKernelGGL(k_copy_guarded, dim3(blas1_grid(c, nd / 2 + 1)), dim3(256), 0, c->stream, (const double *)(xfull + row0 * ED), y, nd, c->guard());
        HIPCHK(hipGetLastError());
        return LK_OK;
    }
};

// ---- dense: the operator's own matrix, or a view of caller memory ---------------------------------------------------------------
constexpr int64_t GEMV_COLS_PER_CHUNK = 256;
struct DenseOp final : lk_linop_s {
    using lk_linop_s::lk_linop_s;
    DevBuf<double> A;
    int64_t lda = 0;
    RowPartition part;
    DevBuf<double> gpart;                    // k_gemv_n's per-chunk partial sums
    int gchunks = 1;
    int apply(int trans, const double *x, double *y, ProfScope &) override {
        const bool cp = dtype == LK_C128;
        if (trans == LK_OP_N) {
            const double *xg = nullptr;
            LKCHK(part.gather_x(ctx, ed(), x, &xg));                                          // sharded: all-gather of x
            const dim3 grid((unsigned)((n + (cp ? 255 : 511)) / (cp ? 256 : 512)), (unsigned)gchunks);
            if (n > 0) {
                const auto gemv_n = cp ? k_gemv_n<true> : k_gemv_n<false>;
                hipLaunchKernelGGL(gemv_n, grid, dim3(256), 0, ctx->stream, A, lda, n, part.ncols_g, xg, gpart, GEMV_COLS_PER_CHUNK, ctx->guard());
                hipLaunchKernelGGL(k_gemv_n_finish, dim3(blas1_grid(ctx, n * ed())), dim3(256), 0, ctx->stream, (const double *)gpart, n * ed(), gchunks, y, ctx->guard());
            }
        } else {
            double *z = part.adjoint_out(ctx, y);
            if (part.ncols_g > 0) {
                const auto gemv_h = cp ? k_gemv_h<true> : k_gemv_h<false>;
                hipLaunchKernelGGL(gemv_h, dim3((unsigned)((part.ncols_g + 3) / 4)), dim3(256), 0, ctx->stream, A, lda, n, part.ncols_g, x, z, ctx->guard());
            }
            LKCHK(part.reduce_to_slice(ctx, ed(), n, y));
        }
        return LK_OK;
    }
};

// ---- CSR: A (for 'N') and its conjugate transpose (for 'H'), both row-compressed ------------------------------------------------
struct CsrOp final : lk_linop_s {
    using lk_linop_s::lk_linop_s;
    RowPartition part;
    struct Csr {
        DevBuf<int64_t> rowptr; DevBuf<int32_t> colind; DevBuf<double> vals; int W = 8;   // W = lanes per row
        DevBuf<int64_t> rowblocks; int64_t nblocks = 0, nnz_hint = 0;   // CSR-stream partition (short rows), see k_csr_stream
    } csr[2];
    // row-sharded, COMPRESSED exchange: only the entries of x that some other rank's rows reference travel.  cx_send_idx =
    // local indices of this rank's entries anybody needs (sorted); every rank's packed entries are all-gathered into cx_xrem
    // (rank r's at cx_displs[r]); the column indices of csr[0] address [own rows | cx_xrem].
    bool cx = false;
    DevBuf<int32_t> cx_send_idx;
    int64_t cx_nsend = 0, cx_total = 0;
    DevBuf<double> cx_sendbuf, cx_xrem;
    std::vector<int64_t> cx_counts, cx_displs;   // in DOUBLES, per rank
    int apply(int trans, const double *x, double *y, ProfScope &) override {
        const bool cp = dtype == LK_C128;
        const bool fwd = trans == LK_OP_N;
        const auto &m = csr[fwd ? 0 : 1];
        const int W = ctx->csr_lanes ? ctx->csr_lanes : m.W;                 // (a forced lane count is never written into the operator)
        const int64_t nr = fwd ? n : part.ncols_g;                       // rows of the product computed here
        const double *xin = x, *xrem = nullptr;
        int64_t nloc = INT64_MAX;                                        // column indices below nloc address `xin`, the others `xrem`
        if (ctx->nranks > 1 && fwd && cx) {
            // compressed exchange: pack what other ranks' rows reference, all-gather the packed pieces, multiply [own rows | pieces]
            if (!ctx->allgather) return fail(LK_ERR_COMM, "row-sharded CSR operator but no all-gather installed (lk_comm_init_rank / lk_set_allgather)");
            if (cx_nsend > 0) {
                const auto pack = cp ? k_pack<true> : k_pack<false>;
                hipLaunchKernelGGL(pack, dim3(blas1_grid(ctx, cx_nsend)), dim3(256), 0, ctx->stream, x, cx_send_idx, cx_nsend, cx_sendbuf, ctx->guard());
                HIPCHK(hipGetLastError());
            }
            {
                ProfScope ps(ctx, "comm_allgather", (double)cx_total * (cp ? 16.0 : 8.0));
                if (ctx->allgather(ctx->allgather_user, cx_sendbuf, cx_xrem, cx_counts.data(), cx_displs.data(), ctx->nranks, (void *)ctx->stream) != 0)
                    return fail(LK_ERR_COMM, "all-gather callback failed");
            }
            xrem = cx_xrem;
            nloc = n;
        } else if (fwd) LKCHK(part.gather_x(ctx, ed(), x, &xin));
        double *yout = fwd ? y : part.adjoint_out(ctx, y);
        auto blocks = [this](int64_t g) {                                // at least one block, at most 16 per CU
            return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(g, (int64_t)ctx->num_cu * 16)));
        };
        if (ctx->csr_stream && nr > 0 && (double)m.nnz_hint / (double)nr <= 32.0 && !ctx->csr_lanes) {
            // short rows: stream the entries through LDS (k_csr_stream)
            const auto stream = cp ? k_csr_stream<true> : k_csr_stream<false>;
            hipLaunchKernelGGL(stream, blocks(m.nblocks), dim3(256), 0, ctx->stream, m.rowblocks, m.rowptr, m.colind, m.vals, xin, yout, m.nblocks, ctx->guard(), xrem, nloc);
        } else {
            // W lanes per row: [log2 W][real]
            static constexpr decltype(&k_csr<true, 1>) rows[7][2] = {
                {k_csr<true, 1>, k_csr<false, 1>}, {k_csr<true, 2>, k_csr<false, 2>}, {k_csr<true, 4>, k_csr<false, 4>}, {k_csr<true, 8>, k_csr<false, 8>},
                {k_csr<true, 16>, k_csr<false, 16>}, {k_csr<true, 32>, k_csr<false, 32>}, {k_csr<true, 64>, k_csr<false, 64>}};
            int lg = 0;
            while (lg < 6 && (1 << lg) < W) ++lg;
            if ((1 << lg) != W) return fail(LK_ERR_INVALID, "internal: CSR lanes per row %d", W);
            const int64_t rows_per_block = 256 / W;
            hipLaunchKernelGGL(rows[lg][cp ? 0 : 1], blocks((nr + rows_per_block - 1) / rows_per_block), dim3(256), 0, ctx->stream, m.rowptr, m.colind, m.vals, xin, yout, nr, ctx->guard(), xrem, nloc);
        }
        HIPCHK(hipGetLastError());
        if (!fwd) LKCHK(part.reduce_to_slice(ctx, ed(), n, y));
        return LK_OK;
    }
};

// ---- the neighbour flags of a sharded stencil (lap5, Ginzburg-Landau) -----------------------------------------------------------
struct Neighbours {
    bool has_lo = false, has_hi = false;     // a neighbouring rank below / above this block
    bool any() const { return has_lo || has_hi; }
    template <class P> P lo(P p) const { return has_lo ? p : P(nullptr); }   // what goes to / comes from below, or NULL
    template <class P> P hi(P p) const { return has_hi ? p : P(nullptr); }
    // the halo exchange addresses its peers by RANK ORDER (rank - 1 below, rank + 1 above): a partition that does not follow
    // it would skip a send on one side and leave the neighbour waiting
    bool follow_rank_order(lk_context_t c) const { return c->nranks <= 1 || (has_lo == (c->rank > 0) && has_hi == (c->rank < c->nranks - 1)); }
};

int halo_exchange(lk_context_t c, const double *send_lo, const double *send_hi, double *recv_lo, double *recv_hi, int64_t count) {
    if (!c->halo) return fail(LK_ERR_COMM, "row-sharded stencil operator but no halo exchange installed (lk_comm_init_rank / lk_set_halo_exchange)");
    ProfScope ps(c, "comm_halo", (double)count * 8.0 * ((send_lo ? 1 : 0) + (send_hi ? 1 : 0)));
    const int rc = c->halo(c->halo_user, send_lo, send_hi, recv_lo, recv_hi, count, (void *)c->stream);
    if (rc != 0) return fail(LK_ERR_COMM, "halo exchange callback returned %d", rc);
    return LK_OK;
}

// ---- lap5: the 5-point Laplacian on NJ grid lines of an N x N grid, real kind ---------------------------------------------------
struct Lap5Op final : lk_linop_s {
    using lk_linop_s::lk_linop_s;
    int64_t N = 0, NJ = 0;                   // grid size; grid lines held by this rank
    Neighbours nb;
    DevBuf<double> halo;                     // 2 N doubles (line from rank-1 | line from rank+1), sharded only
    int apply(int, const double *x, double *y, ProfScope &) override {
        const double s = (double)(N + 1) * (double)(N + 1);
        double *lo = nullptr, *hi = nullptr;
        if (nb.any()) {
            // first / last local grid line to the neighbouring ranks, theirs into the halo buffer (N doubles each)
            lo = nb.lo(halo.get()); hi = nb.hi(halo + N);
            LKCHK(halo_exchange(ctx, nb.lo(x), nb.hi(x + (NJ - 1) * N), lo, hi, N));
        }
        dim3 grid((unsigned)((N / 2 + 1 + 255) / 256), (unsigned)NJ);
        if ((N & 1) == 0) {                               // persistent blocks over (line, segment) tiles
            int64_t tiles = NJ * ((N / 2 + 255) / 256), g = (int64_t)ctx->num_cu * ctx->lap5_grid_mult;
            grid = dim3((unsigned)(tiles < g ? (tiles > 0 ? tiles : 1) : g), 1);
        }
        hipLaunchKernelGGL(k_lap5, grid, dim3(256), 0, ctx->stream, x, y, N, NJ, lo, hi, s, ctx->guard());
        return LK_OK;
    }
};

// ---- Ginzburg-Landau: nsub classical RK4 steps of the linearised equation, complex kind -----------------------------------------
struct GlOp final : lk_linop_s {
    using lk_linop_s::lk_linop_s;
    int64_t row0 = 0, n_global = 0;
    double gl[8] = {0};                      // dx, halfL, nu_re, nu_im, ga_re, ga_im, mu_c, mu2
    double tau = 0; int nsub = 1;
    Neighbours nb;
    DevBuf<double> wk;                       // 3 work vectors (k_a, k_b, u_sub) | halo | edges
    double *halo() const { return wk + (size_t)6 * n; }   // the neighbours' edge values: 4 doubles
    double *edges() const { return halo() + 4; }          // this rank's two edge values (send buffer): 4 doubles
    int apply(int trans, const double *x, double *y, ProfScope &) override {
        const double dt = tau / nsub;                        // 4 stage launches per step
        double *ka = wk, *kb = wk + 2 * n, *us = wk + 4 * n;
        const unsigned grid = (unsigned)((n + 255) / 256);
        const int adj = trans == LK_OP_H;
        const double *uin = x;
        for (int sstep = 0; sstep < nsub; ++sstep) {
            // outputs alternate between the work vector and y so that the LAST sub-step lands in y
            double *uout = ((nsub - 1 - sstep) % 2 == 0) ? y : us;
            auto stage = [&](const double *kprev, double a, double *kout, double b, int first) -> int {
                if (nb.any()) {   // the stage needs v = u + a*kprev one point beyond either end of this rank's block
                    hipLaunchKernelGGL(k_gl_edges, dim3(1), dim3(64), 0, ctx->stream, uin, kprev, a, n, edges(), ctx->guard());
                    LKCHK(halo_exchange(ctx, nb.lo(edges()), nb.hi(edges() + 2), nb.lo(halo()), nb.hi(halo() + 2), 2));
                }
                hipLaunchKernelGGL(k_gl_stage, dim3(grid), dim3(256), 0, ctx->stream, uin, kprev, a, kout, uout, b, first, n, gl[0], gl[1],
                                   gl[2], gl[3], gl[4], gl[5], gl[6], gl[7], adj, row0, n_global, nb.any() ? (const double *)halo() : nullptr, ctx->guard());
                return LK_OK;
            };
            LKCHK(stage(nullptr, 0.0, ka, dt / 6.0, 1));
            LKCHK(stage(ka, 0.5 * dt, kb, dt / 3.0, 0));
            LKCHK(stage(kb, 0.5 * dt, ka, dt / 3.0, 0));
            LKCHK(stage(ka, dt, kb, dt / 6.0, 0));
            uin = uout;
        }
        return LK_OK;
    }
};

// ---- product of two operators: y = op_a(A) op_b(B) x -----------------------------------------------------------------------------
// The factors are NOT owned (they outlive this operator); `apply` only sequences theirs through one scratch vector, so it works
// wherever both factors do (row-sharded contexts included).  The scratch is the operator's own (lk_linop_compose_create), or a view of
// caller memory (lk_gmres: a column of its workspace).  No row-local form: rowop() stays the default.
struct ComposeOp final : lk_linop_s {
    lk_linop_t A, B;
    int ta, tb;
    DevBuf<double> tmp;
    ComposeOp(lk_linop_t a, int transA, lk_linop_t b, int transB) : lk_linop_s(a->ctx, a->dtype, a->n), A(a), B(b), ta(transA ? 1 : 0), tb(transB ? 1 : 0) {
        matvec_bytes = a->matvec_bytes + b->matvec_bytes + 2.0 * n * ed() * 8.0;   // the factors' + scratch written, scratch read
    }
    int apply(int trans, const double *x, double *y, ProfScope &ps) override {
        if (trans == LK_OP_N) {
            LKCHK(B->apply(tb ? LK_OP_H : LK_OP_N, x, tmp, ps));
            HIPCHK(hipGetLastError());
            return A->apply(ta ? LK_OP_H : LK_OP_N, tmp, y, ps);
        }
        LKCHK(A->apply(ta ? LK_OP_N : LK_OP_H, x, tmp, ps));             // (op_a(A) op_b(B))^H = op_b(B)^H op_a(A)^H
        HIPCHK(hipGetLastError());
        return B->apply(tb ? LK_OP_N : LK_OP_H, tmp, y, ps);
    }
};

}  // namespace
}  // extern "C++"

// ---- creators -------------------------------------------------------------------------------------------------------------------
int lk_linop_diag_create(lk_context_t c, int dtype, int64_t n_local, const void *d_host, lk_linop_t *op) {
    if (!c || !d_host || !op) return fail(LK_ERR_INVALID, "lk_linop_diag_create: null argument");
    DevGuard dev_guard(c);
    if (dtype != LK_F64 && dtype != LK_C128) return fail(LK_ERR_INVALID, "bad dtype");
    std::unique_ptr<DiagOp> o(new DiagOp(c, dtype, n_local));
    const int ED = o->ed();
    LKCHK(o->d.reserve((n_local + 2) * ED));
    HIPCHK(hipMemcpy(o->d, d_host, (size_t)n_local * ED * sizeof(double), hipMemcpyHostToDevice));
    *op = o.release();
    return LK_OK;
}

int lk_linop_diag_linspace_create(lk_context_t c, int64_t n_local, int64_t row0, double d0, double dstep, lk_linop_t *op) {
    if (!c || !op) return fail(LK_ERR_INVALID, "null argument");
    std::unique_ptr<DiagLinOp> o(new DiagLinOp(c, n_local));
    o->row0 = row0; o->d0 = d0; o->dstep = dstep;
    *op = o.release();
    return LK_OK;
}

int lk_linop_compose_create(lk_linop_t A, int transA, lk_linop_t B, int transB, lk_linop_t *op) {
    if (!A || !B || !op) return fail(LK_ERR_INVALID, "lk_linop_compose_create: null argument");
    if (A->ctx != B->ctx) return fail(LK_ERR_INVALID, "lk_linop_compose_create: the factors belong to different contexts");
    if (A->dtype != B->dtype) return fail(LK_ERR_INVALID, "lk_linop_compose_create: the factors are of different kinds");
    if (A->n != B->n) return fail(LK_ERR_INVALID, "lk_linop_compose_create: the factors have %lld and %lld rows", (long long)A->n, (long long)B->n);
    DevGuard dev_guard(A->ctx);
    std::unique_ptr<ComposeOp> o(new ComposeOp(A, transA, B, transB));
    LKCHK(o->tmp.reserve((o->n + 2) * o->ed()));
    *op = o.release();
    return LK_OK;
}

// the row-sharded dense operator on `A`: the operator's own matrix, or a view of caller memory
static int dense_build(lk_context_t c, int dtype, int64_t n_global, const int64_t *row_starts, DevBuf<double> A, int64_t lda, lk_linop_t *op) {
    if (((uintptr_t)(double *)A & 15) != 0) return fail(LK_ERR_INVALID, "lk_linop_dense_wrap_sharded: pointer must be 16-byte aligned");
    if (dtype == LK_F64 && (lda & 1)) return fail(LK_ERR_INVALID, "lk_linop_dense_wrap_sharded: lda must be even for LK_F64");
    std::unique_ptr<DenseOp> o(new DenseOp(c, dtype, 0));
    o->A = std::move(A); o->lda = lda;
    LKCHK(o->part.shard_setup(c, o->ed(), n_global, row_starts, "lk_linop_dense_wrap_sharded", &o->n));
    if (lda < o->n) return fail(LK_ERR_INVALID, "lk_linop_dense_wrap_sharded: lda < local rows");
    // split-K of y = A x in chunks of GEMV_COLS_PER_CHUNK columns: the chunking depends on the GLOBAL column count only, so a
    // row's products are added in the same order whatever the row partition (sharded matvec = single-rank matvec bit for bit)
    o->gchunks = (int)std::max<int64_t>(1, (n_global + GEMV_COLS_PER_CHUNK - 1) / GEMV_COLS_PER_CHUNK);
    LKCHK(o->gpart.reserve((int64_t)o->gchunks * (o->n > 0 ? o->n : 1) * o->ed()));
    *op = o.release();
    return LK_OK;
}

int lk_linop_dense_wrap_sharded(lk_context_t c, int dtype, int64_t n_global, const int64_t *row_starts, void *dev_ptr, int64_t lda,
                                lk_linop_t *op) {
    if (!c || !dev_ptr || !op) return fail(LK_ERR_INVALID, "lk_linop_dense_wrap_sharded: null argument");
    DevGuard dev_guard(c);
    if (dtype != LK_F64 && dtype != LK_C128) return fail(LK_ERR_INVALID, "bad dtype");
    DevBuf<double> A;
    A.wrap((double *)dev_ptr);
    return dense_build(c, dtype, n_global, row_starts, std::move(A), lda, op);
}

int lk_linop_dense_create_sharded(lk_context_t c, int dtype, int64_t n_global, const int64_t *row_starts, const void *A_rows, int64_t lda,
                                  lk_linop_t *op) {
    if (!c || !A_rows || !op || !row_starts) return fail(LK_ERR_INVALID, "lk_linop_dense_create_sharded: null argument");
    DevGuard dev_guard(c);
    if (dtype != LK_F64 && dtype != LK_C128) return fail(LK_ERR_INVALID, "bad dtype");
    const int64_t n_local = row_starts[c->rank + 1] - row_starts[c->rank];
    if (n_local < 0 || lda < n_local) return fail(LK_ERR_INVALID, "lk_linop_dense_create_sharded: lda < local rows");
    const size_t es = (dtype == LK_C128 ? 2 : 1) * sizeof(double);
    const int64_t ldd = ((n_local + 31) / 32) * 32 + (n_local == 0 ? 32 : 0);          // 256-byte columns on the device
    DevBuf<double> dev;
    LKCHK(dev.reserve(ldd * (n_global > 0 ? n_global : 1) * (dtype == LK_C128 ? 2 : 1)));
    if (n_local > 0 && n_global > 0)
        HIPCHK(hipMemcpy2D(dev, (size_t)ldd * es, A_rows, (size_t)lda * es, (size_t)n_local * es, n_global, hipMemcpyHostToDevice));
    return dense_build(c, dtype, n_global, row_starts, std::move(dev), ldd, op);
}

int lk_linop_dense_create(lk_context_t c, int dtype, int64_t n, const void *A_host, int64_t lda, lk_linop_t *op) {
    if (!c || !A_host || !op) return fail(LK_ERR_INVALID, "lk_linop_dense_create: null argument");
    if (lda < n) return fail(LK_ERR_INVALID, "lda < n");
    if (c->nranks > 1) return fail(LK_ERR_INVALID, "dense_linop over several ranks: use lk_linop_dense_create_sharded (a row block per rank)");
    const int64_t starts[2] = {0, n};
    return lk_linop_dense_create_sharded(c, dtype, n, starts, A_host, lda, op);
}

int lk_linop_lap5_create_sharded(lk_context_t c, int64_t N, int64_t j0, int64_t nj, lk_linop_t *op) {
    if (!c || !op || N < 1 || j0 < 0 || nj < 1 || j0 + nj > N) return fail(LK_ERR_INVALID, "lk_linop_lap5_create: bad argument");
    DevGuard dev_guard(c);
    std::unique_ptr<Lap5Op> o(new Lap5Op(c, LK_F64, nj * N));
    o->N = N; o->NJ = nj;
    o->nb.has_lo = j0 > 0; o->nb.has_hi = j0 + nj < N;
    if (!o->nb.follow_rank_order(c))
        return fail(LK_ERR_INVALID, "lk_linop_lap5_create_sharded: grid lines [%lld, %lld) of %lld on rank %d/%d do not follow rank order "
                    "(rank r must own the r-th consecutive block)", (long long)j0, (long long)(j0 + nj), (long long)N, c->rank, c->nranks);
    if (o->nb.any()) LKCHK(o->halo.reserve(2 * N));
    *op = o.release();
    return LK_OK;
}

int lk_linop_lap5_create(lk_context_t c, int64_t N, lk_linop_t *op) {
    if (c && c->nranks > 1) return fail(LK_ERR_INVALID, "lap5 over several ranks: use lk_linop_lap5_create_sharded (grid lines per rank)");
    return lk_linop_lap5_create_sharded(c, N, 0, N, op);
}

int lk_linop_gl_create_sharded(lk_context_t c, int64_t n_global, int64_t row0, int64_t n_local, double dx, double tau, int nsub,
                               const double *nu, const double *gamma, double mu_c, double mu2, lk_linop_t *op) {
    if (!c || !op || !nu || !gamma || n_global < 1 || n_local < 1 || row0 < 0 || row0 + n_local > n_global || nsub < 1 || !(dx > 0.0))
        return fail(LK_ERR_INVALID, "lk_linop_gl_create: bad argument");
    DevGuard dev_guard(c);
    std::unique_ptr<GlOp> o(new GlOp(c, LK_C128, n_local));
    o->tau = tau; o->nsub = nsub; o->row0 = row0; o->n_global = n_global;
    o->nb.has_lo = row0 > 0; o->nb.has_hi = row0 + n_local < n_global;
    if (!o->nb.follow_rank_order(c))
        return fail(LK_ERR_INVALID, "lk_linop_gl_create_sharded: rows [%lld, %lld) of %lld on rank %d/%d do not follow rank order "
                    "(rank r must own the r-th consecutive block)", (long long)row0, (long long)(row0 + n_local), (long long)n_global, c->rank, c->nranks);
    o->gl[0] = dx; o->gl[1] = 0.5 * dx * (double)(n_global + 1);   // L = dx (n+1), x = linspace(-L/2, L/2, n+2)
    o->gl[2] = nu[0]; o->gl[3] = nu[1]; o->gl[4] = gamma[0]; o->gl[5] = gamma[1]; o->gl[6] = mu_c; o->gl[7] = mu2;
    LKCHK(o->wk.reserve(3 * n_local * 2 + 8));
    (void)hipMemsetAsync(o->halo(), 0, 8 * sizeof(double), c->stream);
    *op = o.release();
    return LK_OK;
}

int lk_linop_gl_create(lk_context_t c, int64_t n, double dx, double tau, int nsub, const double *nu, const double *gamma,
                       double mu_c, double mu2, lk_linop_t *op) {
    if (c && c->nranks > 1) return fail(LK_ERR_INVALID, "Ginzburg-Landau operator over several ranks: use lk_linop_gl_create_sharded");
    return lk_linop_gl_create_sharded(c, n, 0, n, dx, tau, nsub, nu, gamma, mu_c, mu2, op);
}

// A = (rowptr, colind, vals) in CSR, 0-based; `which` = 0 stores A itself, 1 its conjugate transpose (built on the host by a
// counting sort: column indices within a row of A^H come out ascending, so both products sum in index order).
static int csr_upload(CsrOp *o, int which, int64_t n, const int64_t *rowptr, const int32_t *colind, const double *vals, int ED) {
    const int64_t nnz = rowptr[n];
    auto &m = o->csr[which];
    LKCHK(m.rowptr.reserve(n + 1));
    LKCHK(m.colind.reserve(nnz > 0 ? nnz : 1));
    LKCHK(m.vals.reserve((nnz > 0 ? nnz : 1) * ED));
    HIPCHK(hipMemcpy(m.rowptr, rowptr, (size_t)(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nnz > 0) {
        HIPCHK(hipMemcpy(m.colind, colind, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(m.vals, vals, (size_t)nnz * ED * sizeof(double), hipMemcpyHostToDevice));
    }
    {   // CSR-stream partition: consecutive rows, at most CSR_NNZ entries and 256 rows per block; a longer row stands alone
        std::vector<int64_t> rb;
        rb.push_back(0);
        int64_t r = 0;
        while (r < n) {
            int64_t e = r + 1;                                              // at least one row, however long
            while (e < n && e - r < 256 && rowptr[e + 1] - rowptr[r] <= CSR_NNZ) ++e;
            rb.push_back(e);
            r = e;
        }
        m.nblocks = (int64_t)rb.size() - 1;
        LKCHK(m.rowblocks.reserve((int64_t)rb.size()));
        HIPCHK(hipMemcpy(m.rowblocks, rb.data(), rb.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    m.nnz_hint = nnz;
    const double mean = n > 0 ? (double)nnz / (double)n : 0.0;
    int W = 1;                                   // lanes per row: the power of two at or below half the mean row length
    while (W < 64 && 2 * W <= mean / 2.0) W <<= 1;   // (5-point Laplacian, n = 1.7e7: W = 1 / 2 / 4 / 8 / 16 -> see DESIGN.md)
    m.W = W;
    return LK_OK;
}

// creation-time metadata exchange through the data-path hook: every rank contributes `mine` (counts[rank] doubles), all receive all
static int host_allgatherv(lk_context_t c, const std::vector<double> &mine, const std::vector<int64_t> &counts, std::vector<double> &all) {
    std::vector<int64_t> displs(c->nranks, 0);
    int64_t total = 0;
    for (int r = 0; r < c->nranks; ++r) { displs[r] = total; total += counts[r]; }
    all.assign((size_t)total, 0.0);
    if (total == 0) return LK_OK;
    if (!c->allgather) return fail(LK_ERR_COMM, "row-sharded CSR operator but no all-gather installed (lk_comm_init_rank / lk_set_allgather)");
    DevBuf<double> ds, dr;
    LKCHK(ds.reserve(mine.size() > 0 ? (int64_t)mine.size() : 1));
    LKCHK(dr.reserve(total));
    int rc = LK_OK;
    if (!mine.empty() && hipMemcpyAsync(ds, mine.data(), mine.size() * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail(LK_ERR_HIP, "metadata upload failed");
    if (rc == LK_OK && c->allgather(c->allgather_user, ds, dr, counts.data(), displs.data(), c->nranks, (void *)c->stream) != 0)
        rc = fail(LK_ERR_COMM, "all-gather callback failed (metadata)");
    if (rc == LK_OK && hipMemcpyAsync(all.data(), dr, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail(LK_ERR_HIP, "metadata download failed");
    if (rc == LK_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(LK_ERR_HIP, "stream synchronisation failed");
    return rc;
}

// A COLLECTIVE creation routine must not leave a rank behind: a rank that returned early (a bad column index, a failed
// allocation) would let the others wait for it in the next exchange for ever.  Every rank contributes its local status; when any
// rank failed, EVERY rank returns an error -- its own where it has one, otherwise one naming the first rank that failed.  One
// tiny all-gather through the data-path hook + a stream synchronisation: creation time only.
static int agree_status(lk_context_t c, int rc_local, const char *what) {
    if (c->nranks <= 1) return rc_local;
    std::vector<double> mine(1, (double)rc_local), all;
    const int xrc = host_allgatherv(c, mine, std::vector<int64_t>((size_t)c->nranks, 1), all);
    if (xrc != LK_OK) return rc_local != LK_OK ? rc_local : xrc;
    if (rc_local != LK_OK) return rc_local;                   // lk_last_error already says why
    for (int r = 0; r < c->nranks; ++r)
        if (all[(size_t)r] != 0.0)
            return fail(LK_ERR_COMM, "%s: rank %d failed (status %d); every rank returns without the operator", what, r, (int)all[(size_t)r]);
    return LK_OK;
}

// Decide and set up the compressed exchange of a row-sharded CSR operator (COLLECTIVE: every rank calls it at creation).  On
// return `cols` holds the column indices csr[0] is uploaded with: remapped to [own rows | packed remote entries] when o->cx, the
// global ones otherwise.  The exchange is compressed when what travels is less than half of x (stencils, banded matrices: a few
// boundary entries per neighbour); matrices whose rows reach everywhere keep the plain all-gather of x.
static int csr_compress_setup(CsrOp *o, lk_context_t c, const int64_t *row_starts, int64_t n, const int64_t *rowptr, const int32_t *colind,
                              std::vector<int32_t> &cols) {
    const int P = c->nranks, me = c->rank;
    const int ED = o->ed();
    const int64_t nnz = rowptr[n], row0 = row_starts[me], n_global = row_starts[P];
    cols.assign(colind, colind + nnz);
    if (P == 1) return LK_OK;
    auto owner = [&](int64_t j) {                        // rank whose block holds global row j
        int lo = 0, hi = P - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) / 2; if (row_starts[mid] <= j) lo = mid; else hi = mid - 1; }
        while (lo + 1 < P && row_starts[lo + 1] <= j) ++lo;      // empty blocks share a start
        return lo;
    };
    // what I need from whom: the out-of-block column indices, sorted and unique -- owners hold contiguous row ranges, so the
    // sorted list falls apart into one run per owner (4 bytes per remote entry of transient memory, no per-owner vectors)
    std::vector<int32_t> rem;
    for (int64_t p = 0; p < nnz; ++p) {
        const int64_t j = colind[p];
        if (j < row0 || j >= row0 + n) rem.push_back((int32_t)j);
    }
    std::sort(rem.begin(), rem.end());
    rem.erase(std::unique(rem.begin(), rem.end()), rem.end());
    std::vector<std::vector<int64_t>> need(P);
    for (int32_t j : rem) need[owner(j)].push_back(j);
    std::vector<int32_t>().swap(rem);
    // everybody learns everybody's request COUNTS (a P x P table); the lists themselves travel only when the compressed exchange
    // can still pay off: what anybody needs of rank r's block is at least the longest single request for it, so
    // 2 * sum_r max_q count[q][r] >= n_global already means "half of x or more travels anyway" -- decided from the table every
    // rank holds identically, before the O(P * requests) exchange of the lists (matrices whose rows reach widely)
    std::vector<double> mycnt(P), allcnt;
    for (int r = 0; r < P; ++r) mycnt[r] = (double)need[r].size();
    LKCHK(host_allgatherv(c, mycnt, std::vector<int64_t>(P, P), allcnt));
    int64_t maxn = 0;
    for (int r = 0; r < P; ++r) maxn = std::max(maxn, row_starts[r + 1] - row_starts[r]);
    {
        int64_t lower = 0;
        for (int r = 0; r < P; ++r) {
            int64_t mx = 0;
            for (int q = 0; q < P; ++q) mx = std::max(mx, (int64_t)allcnt[(size_t)q * P + r]);
            lower += mx;
        }
        if (2 * lower >= n_global) return LK_OK;
    }
    std::vector<int64_t> listlen(P, 0);
    for (int q = 0; q < P; ++q) for (int r = 0; r < P; ++r) listlen[q] += (int64_t)allcnt[(size_t)q * P + r];
    std::vector<double> mylist, alllist;
    for (int r = 0; r < P; ++r) for (int64_t j : need[r]) mylist.push_back((double)j);
    LKCHK(host_allgatherv(c, mylist, listlen, alllist));
    // S_r = what anybody needs of rank r's block (sorted, unique): the packed buffer rank r contributes per matvec
    std::vector<std::vector<int64_t>> S(P);
    {
        size_t pos = 0;
        for (int q = 0; q < P; ++q)
            for (int r = 0; r < P; ++r) {
                const int64_t cnt = (int64_t)allcnt[(size_t)q * P + r];
                for (int64_t i = 0; i < cnt; ++i) S[r].push_back((int64_t)alllist[pos + (size_t)i]);
                pos += (size_t)cnt;
            }
        for (auto &v : S) { std::sort(v.begin(), v.end()); v.erase(std::unique(v.begin(), v.end()), v.end()); }
    }
    int64_t total = 0;
    for (int r = 0; r < P; ++r) total += (int64_t)S[r].size();
    // nearly all of x travels anyway, or the remapped indices would not fit: plain all-gather.  Decided from quantities every rank
    // holds identically (a rank that chose differently would issue a different collective)
    if (2 * total >= n_global || maxn + total > 2147483647LL) return LK_OK;
    o->cx = true;
    o->cx_total = total;
    o->cx_counts.resize(P); o->cx_displs.resize(P);
    std::vector<int64_t> off(P, 0);
    { int64_t a = 0; for (int r = 0; r < P; ++r) { off[r] = a; o->cx_counts[r] = (int64_t)S[r].size() * ED; o->cx_displs[r] = a * ED; a += (int64_t)S[r].size(); } }
    for (int64_t p = 0; p < nnz; ++p) {
        const int64_t j = colind[p];
        if (j >= row0 && j < row0 + n) { cols[(size_t)p] = (int32_t)(j - row0); continue; }
        const int r = owner(j);
        const int64_t k = std::lower_bound(S[r].begin(), S[r].end(), j) - S[r].begin();
        cols[(size_t)p] = (int32_t)(n + off[r] + k);
    }
    o->cx_nsend = (int64_t)S[me].size();
    std::vector<int32_t> sidx((size_t)(o->cx_nsend > 0 ? o->cx_nsend : 1), 0);
    for (int64_t i = 0; i < o->cx_nsend; ++i) sidx[(size_t)i] = (int32_t)(S[me][(size_t)i] - row0);
    LKCHK(o->cx_send_idx.reserve((int64_t)sidx.size()));
    HIPCHK(hipMemcpy(o->cx_send_idx, sidx.data(), sidx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    LKCHK(o->cx_sendbuf.reserve((o->cx_nsend > 0 ? o->cx_nsend : 1) * ED));
    return o->cx_xrem.reserve((total > 0 ? total : 1) * ED);
}

// local (rank-private) validation of a row block: nothing here talks to another rank
static int csr_validate_rows(lk_context_t c, int dtype, int64_t n_global, const int64_t *row_starts, const int64_t *rowptr, const int32_t *colind,
                             const void *vals) {
    if (!rowptr) return fail(LK_ERR_INVALID, "lk_linop_csr_create: null rowptr (this rank's row block was rejected by the caller)");
    if (dtype != LK_F64 && dtype != LK_C128) return fail(LK_ERR_INVALID, "lk_linop_csr_create: bad dtype %d", dtype);
    if (n_global < 0 || n_global > 2147483647LL) return fail(LK_ERR_INVALID, "lk_linop_csr_create: bad size %lld", (long long)n_global);
    const int64_t n = row_starts[c->rank + 1] - row_starts[c->rank];      // rows held here; column indices are GLOBAL
    if (n < 0) return fail(LK_ERR_INVALID, "lk_linop_csr_create: row_starts decreases");
    if (rowptr[0] != 0) return fail(LK_ERR_INVALID, "lk_linop_csr_create: rowptr must be 0-based");
    for (int64_t i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(LK_ERR_INVALID, "lk_linop_csr_create: rowptr decreases at row %lld", (long long)i);
    const int64_t nnz = rowptr[n];
    if (nnz > 0 && (!colind || !vals)) return fail(LK_ERR_INVALID, "lk_linop_csr_create: null colind / vals");
    for (int64_t p = 0; p < nnz; ++p)
        if (colind[p] < 0 || colind[p] >= n_global) return fail(LK_ERR_INVALID, "lk_linop_csr_create: column index %d out of range at entry %lld", colind[p], (long long)p);
    return LK_OK;
}

int lk_linop_csr_create_sharded(lk_context_t c, int dtype, int64_t n_global, const int64_t *row_starts, const int64_t *rowptr,
                                const int32_t *colind, const void *vals, lk_linop_t *op) {
    // a null context / result / partition is a programming error of the call site, identical on every rank: plain early return.
    // A null rowptr is NOT: it is how a host-side wrapper that found this rank's input unusable (wrong number of rows, wrong
    // value type) still joins the agreement below, so that every rank fails together (lightkrylov_amd/linops.py).
    if (!c || !op || !row_starts) return fail(LK_ERR_INVALID, "lk_linop_csr_create: null argument");
    DevGuard dev_guard(c);
    // COLLECTIVE from here on.  Everything that can fail on ONE rank only (this rank's rows, this rank's allocations) is agreed
    // on before the next exchange is entered: first the validation of the row block ...
    LKCHK(agree_status(c, csr_validate_rows(c, dtype, n_global, row_starts, rowptr, colind, vals), "lk_linop_csr_create_sharded (validation)"));
    const int64_t n = row_starts[c->rank + 1] - row_starts[c->rank];
    const int64_t nnz = rowptr[n];
    const int ED = dtype == LK_C128 ? 2 : 1;
    const double *v = (const double *)vals;
    // conjugate transpose of the row block (n_global rows, LOCAL column indices) by counting sort over the column indices.  Host
    // allocations of THIS rank (n_global + nnz entries): a bad_alloc must neither cross the C ABI nor leave the peers in the next
    // exchange -- it becomes this rank's status in the "buffers" agreement below
    std::vector<int64_t> tp;
    std::vector<int32_t> tc;
    std::vector<double> tv;
    std::unique_ptr<CsrOp> o;
    int rc_host = LK_OK;
    try {
        tp.assign((size_t)n_global + 1, 0);
        for (int64_t p = 0; p < nnz; ++p) tp[(size_t)colind[p] + 1] += 1;
        for (int64_t j = 0; j < n_global; ++j) tp[(size_t)j + 1] += tp[(size_t)j];
        tc.resize((size_t)(nnz > 0 ? nnz : 1));
        tv.resize((size_t)(nnz > 0 ? nnz : 1) * ED);
        std::vector<int64_t> next(tp.begin(), tp.end() - 1);
        for (int64_t i = 0; i < n; ++i)
            for (int64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) {
                const int64_t q = next[(size_t)colind[p]]++;
                tc[(size_t)q] = (int32_t)i;
                tv[(size_t)q * ED] = v[p * ED];
                if (ED == 2) tv[(size_t)q * 2 + 1] = -v[p * 2 + 1];
            }
        o.reset(new CsrOp(c, dtype, 0));
    } catch (const std::exception &e) {
        rc_host = fail(LK_ERR_NOMEM, "lk_linop_csr_create_sharded: host allocation failed while transposing this rank's rows (%s)", e.what());
    }
    // ... then this rank's share of the set-up that precedes the metadata exchange (the transpose above, the gathered-x buffer) ...
    int rc = agree_status(c, rc_host != LK_OK ? rc_host : o->part.shard_setup(c, ED, n_global, row_starts, "lk_linop_csr_create", &o->n), "lk_linop_csr_create_sharded (buffers)");
    if (rc == LK_OK) {
        // ... the metadata exchange itself (its decisions come from quantities every rank holds identically; its staging buffers
        // are a few P-length tables and the request lists -- a rank that cannot allocate THOSE is fatal for the job, see header) ...
        try {
            std::vector<int32_t> cols0;
            rc = csr_compress_setup(o.get(), c, row_starts, n, rowptr, colind, cols0);
            if (rc == LK_OK) rc = csr_upload(o.get(), 0, n, rowptr, cols0.data(), v, ED);
            if (rc == LK_OK) rc = csr_upload(o.get(), 1, n_global, tp.data(), tc.data(), tv.data(), ED);
        } catch (const std::exception &e) {
            rc = fail(LK_ERR_NOMEM, "lk_linop_csr_create_sharded: host allocation failed (%s)", e.what());
        }
        // ... and finally the uploads: an operator exists on every rank or on none
        rc = agree_status(c, rc, "lk_linop_csr_create_sharded (upload)");
    }
    if (rc != LK_OK) return rc;
    *op = o.release();
    return LK_OK;
}

int lk_linop_csr_create(lk_context_t c, int dtype, int64_t n, const int64_t *rowptr, const int32_t *colind, const void *vals,
                        lk_linop_t *op) {
    if (!c || !rowptr || !op) return fail(LK_ERR_INVALID, "lk_linop_csr_create: null argument");
    if (c->nranks > 1) return fail(LK_ERR_INVALID, "lk_linop_csr_create over several ranks: use lk_linop_csr_create_sharded (a row block per rank)");
    const int64_t starts[2] = {0, n};
    return lk_linop_csr_create_sharded(c, dtype, n, starts, rowptr, colind, vals, op);
}

int lk_linop_destroy(lk_linop_t op) { delete op; return LK_OK; }

int lk_linop_apply(lk_linop_t op, int trans, lk_basis_t Bx, int jx, lk_basis_t By, int jy) {
    if (!op) return fail(LK_ERR_INVALID, "lk_linop_apply: null operator");
    DevGuard dev_guard(op->ctx);
    LKCHK(check_vec(Bx, jx, "lk_linop_apply(vec_in)"));
    LKCHK(check_vec(By, jy, "lk_linop_apply(vec_out)"));
    LKCHK(check_pair(Bx, By, "lk_linop_apply"));
    if (Bx->dtype != op->dtype || Bx->n != op->n) return fail(LK_ERR_INVALID, "lk_linop_apply: operator/vector mismatch");
    lk_context_t c = op->ctx;
    const double *x = Bx->col(jx);
    double *y = By->col(jy);
    if (cols_overlap(Bx, jx, 1, By, jy, 1)) return fail(LK_ERR_INVALID, "lk_linop_apply: vec_in and vec_out alias");
    const VecRef w{By, jy}, r{Bx, jx};
    LKCHK(lazy_enter_vec(c, &w, true, &r, nullptr));           // vec_out is intent(out): AbstractLinops.fypp:74-87
    By->touch(jy);
    ProfScope ps(c, "matvec", op->matvec_bytes, op->one_kernel && c->prof_ext);
    LKCHK(op->apply(trans, x, y, ps));
    HIPCHK(hipGetLastError());
    return LK_OK;
}
