// rlc_host.hpp -- host orchestration of the randomised (small-exponent) batch verifications: blsmi_g?pubs_*verify*_batch_rlc, ..._rlc_grouped,
// ..._rlc_locate, ..._rlc_grouped_locate, the committee aggregates' ..._common*_batch_rlc, blsmi_pairing_product_batch_rlc* and ..._rlc_locate*,
// blsmi_fr_wsum_segmented_u64*, blsmi_groth16_verify_batch*, blsmi_g1_mul_add_batch*, blsmi_kzg_verify_batch*, blsmi_fr_mul_batch*, blsmi_fr_inv_batch*,
// blsmi_fr_eval_batch*, blsmi_kzg_verify_blob_batch*, blsmi_fr_coset_interp_batch*, blsmi_kzg_verify_cell_batch*, blsmi_kzg_blob_challenge_batch* and
// blsmi_kzg_verify_blob_batch_wire*.  Included by blsmi.hip after verify_host.inc, whose aggregate, segmented-sum and pairing-product machinery it calls.  The
// forms are built from one set of stages (RlcCall and the rlc_* functions below); each driver writes out only the stages that are its own.
// Host code only, no kernel in it -- hence not an .inc: the digest of the kernel sources that dates the committed counters (bench.py:
// source_digest) takes every .inc it does not list by name, and a change here cannot make a counter stale.
namespace {
// ---- randomised batch verification (blsmi 0.8: blsmi_g?pubs_verify_batch_rlc) ------------------------------------------------------
// Small-exponent batch verification (Bellare, Garay, Rabin 1998): with random nonzero 64-bit r_i, ONE equation stands for the n of a batch --
//     g2pubs: e(sum r_i sig_i, G2gen) == prod e(r_i H(m_i), pk_i)        g1pubs: e(G1gen, sum r_i sig_i) == prod e(r_i pk_i, H(m_i))
// It holds when every tuple is valid; with an invalid tuple among them it holds with probability at most 2^-64 over the r_i (keys and
// signatures in the prime-order subgroups, as Deserialize guarantees).  n Miller loops, the product tree and ONE final exponentiation (the
// VerifyAggregate machinery), plus a 64-bit multiplication per tuple (k_g1_mul_u64: r_i H_i for g2pubs, r_i pk_i for g1pubs -- both in G1)
// and a 64-bit MSM over the signatures, which runs on the side stream beside the hash.  When the check fails, or a point at infinity
// meets it, the shard computes the per-tuple verdicts of verify_batch from the buffers already on the device.
//
// The scalars: nonzero 64-bit words from the OS (getrandom, /dev/urandom), fresh for every call; no state is kept between calls.
int rlc_draw_scalars(uint64_t* r, size_t n) {
    uint8_t* p = reinterpret_cast<uint8_t*>(r);
    size_t want = 8 * n, got = 0;
#ifdef SYS_getrandom
    while (got < want) {
        const long k = syscall(SYS_getrandom, p + got, std::min(want - got, (size_t)1 << 20), 0);
        if (k > 0) got += (size_t)k;
        else if (k < 0 && errno == EINTR) continue;
        else break;
    }
#endif
    if (got < want) {
        const int fd = open("/dev/urandom", O_RDONLY | O_CLOEXEC);
        if (fd < 0) return BLSMI_E_RNG;
        while (got < want) {
            const ssize_t k = read(fd, p + got, want - got);
            if (k > 0) got += (size_t)k;
            else if (k < 0 && errno == EINTR) continue;
            else break;
        }
        close(fd);
        if (got < want) return BLSMI_E_RNG;
    }
    for (size_t i = 0; i < n; i++)                                         // a zero word (probability 2^-64 each) is drawn again
        while (r[i] == 0) { int rc = rlc_draw_scalars(&r[i], 1); if (rc) return rc; }
    return BLSMI_OK;
}
// The signature side's sum, sum_i r_i sig_i over the n signatures on the device (any curve points): affine at d_sum, infinity flag (int32)
// at d_flag, on g_stream.  From RLC_MSM_BUCKET_MIN signatures the bucket method of msm_bucket_dev over the scalars' 64 bits (four
// 16-bit windows); below, or when the digits are skewed (a caller's scalars), per-signature 64-bit ladders and the tree sum.
constexpr size_t RLC_MSM_BUCKET_MIN = 8192;
int rlc_sig_sum(const GroupKernels& g, const u8* d_sigs, const u64* d_r, size_t n, u8* d_sum, i32* d_flag) {
    hipStream_t s = g_stream;
    if (n >= RLC_MSM_BUCKET_MIN) {
        DBuf sc; HIPCHK(sc.alloc((size_t)32 * n));
        launch_quiet(KERNEL_OF(k_scalar_u64_to_be32), nblocks(n), s, d_r, sc.p, n);
        const int rc = msm_bucket_dev(g, d_sigs, sc.as<u8>(), n, d_sum, d_flag, s, 64);
        if (rc != BLSMI_E_SKEW) return rc;
    }
    DBuf m, inf; HIPCHK(m.alloc(g.wire_bytes * n)); HIPCHK(inf.alloc(n));
    launch(g.mul_u64, nblocks(n), s, d_sigs, d_r, m.p, inf.p, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return sum_dev(g, m.as<u8>(), inf.as<u8>(), n, d_sum, d_flag, s, false);
}
// sig_side_start for a signature already on the device (the sum above, read in place): MillerLoop(-sig, G2gen) / MillerLoop(-G1gen, sig)
// into ss.ml, on g_stream, which the caller has pointed at the side stream; join[0] marks its end for aggregate_tail
int sig_side_start_dev(int kind, const u8* d_sig, SigSide& ss) {
    HIPCHK(ss.ml.alloc(sizeof(i32) * 12 * NL));
    prof_mark(lat_mark(LAT_MILLER1RAWN_OFFSET));
    launch_sig_miller(sig_pair(kind, d_sig, 0), ss.ml.p, 1, g_stream);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(tl_ctx->join[0], g_stream));
    return BLSMI_OK;
}
// the context's stream pointed at another of its streams for a stretch of one call (the kernels and their profile marks go there)
struct OnStream { hipStream_t saved; explicit OnStream(hipStream_t s) : saved(tl_ctx->stream) { tl_ctx->stream = s; } ~OnStream() { tl_ctx->stream = saved; } };

// ---- the stages the three forms share ---------------------------------------------------------------------------------------------------
// The arguments every form checks alike; its own checks that end in BLSMI_E_ARG for a call of n > 0 tuples arrive folded into inputs_ok.
int rlc_check_args(bool inputs_ok, const uint64_t* scalars, size_t n) {
    if (n && !inputs_ok) return BLSMI_E_ARG;
    if (scalars) for (size_t i = 0; i < n; i++) if (scalars[i] == 0) return BLSMI_E_ARG;
    return BLSMI_OK;
}
// The host memory a call may need: the scalars where the caller gave none (drawn here: `scalars` then points at them), and the n verdict
// bytes of a caller who wants the bitmap alone (want_ok: `ok` then points at them).
struct RlcHostScratch { std::vector<uint64_t> drawn; std::vector<uint8_t> tmp; };
int rlc_scalars_and_ok(RlcHostScratch& hs, const uint64_t*& scalars, uint8_t*& ok, bool want_ok, size_t n) {
    try {
        if (!scalars) hs.drawn.resize(n);
        if (want_ok) hs.tmp.resize(n);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    if (want_ok) ok = hs.tmp.data();
    if (!scalars) { int rc = rlc_draw_scalars(hs.drawn.data(), n); if (rc) return rc; scalars = hs.drawn.data(); }
    return BLSMI_OK;
}
// What one combined check keeps for the length of its call.  On the device: the inputs, the verdict bytes, the inputs' flag bytes, the word
// `any` that every flagging kernel ORs into, the signatures' sum and its infinity flag.  On the host: the signature side's Miller value and
// the three words the check ends in -- targets of asynchronous copies, so the struct stays where it is until the call has synchronised.
// A buffer that a later stage reads belongs here or in the driver's frame, never in a stage's.
struct RlcCall {
    int kind = 0;
    Kind k{};
    size_t n = 0;
    bool has_inf = false;                                                  // the caller passed infinity flags (rlc_upload_keys)
    DevMsgs msgs;                                                          // (of the messages that are hashed: n, or a grouped call's d')
    DBuf dp, ds, di, dr, dok, flags, any, sum, sflag;
    SigSide ss;
    int bad = 0, sum_inf = 0, verdict = 0;
    const void* inf() const { return has_inf ? di.p : nullptr; }
    // the equation holds, nothing is flagged, the signatures' sum is a finite point: every verdict is 1
    bool held() const { return verdict == 1 && bad == 0 && sum_inf == 0; }
};
// the context's side streams, and the buffers for n tuples over nmsg messages with the host offsets off_or_domain
int rlc_begin(RlcCall& c, int kind, size_t n, const void* off_or_domain, size_t nmsg) {
    c.kind = kind; c.k = kind_of(kind); c.n = n; c.msgs = DevMsgs(kind, off_or_domain, nmsg);
    HIPCHK(tl_ctx->ensure_aux());
    { int rc = c.msgs.alloc(); if (rc) return rc; }
    HIPCHK(c.dp.alloc((size_t)c.k.pk_bytes * n)); HIPCHK(c.ds.alloc((size_t)c.k.sig_bytes * n));
    HIPCHK(c.di.alloc(n)); HIPCHK(c.dr.alloc(sizeof(uint64_t) * n)); HIPCHK(c.dok.alloc(n)); HIPCHK(c.flags.alloc(n)); HIPCHK(c.any.alloc(sizeof(int)));
    HIPCHK(c.sum.alloc(c.k.sig_bytes)); HIPCHK(c.sflag.alloc(sizeof(i32)));
    return BLSMI_OK;
}
// The uploads a call starts with.  The signatures go first, on the side stream aux[0] (pageable copies block the host: the hash is queued
// behind the first of them only), and join[1] marks their arrival.  The scalars r, the messages and their offsets (or the domain) follow on the
// main stream, where `fork` says that the scalars are there: the side stream's sum may start.
int rlc_upload_start(RlcCall& c, const uint8_t* sigs, const uint64_t* r, const void* msgs, const void* off_or_domain, int fmt) {
    hipStream_t s = g_stream, st = tl_ctx->aux[0];
    { int rc = upload_points(c.k.sig(), (fmt & FMT_SIG_JAC) != 0, sigs, c.ds.p, c.n, st); if (rc) return rc; }
    HIPCHK(hipEventRecord(tl_ctx->join[1], st));
    HIPCHK(hipMemcpyAsync(c.dr.p, r, sizeof(uint64_t) * c.n, hipMemcpyHostToDevice, s));
    { int rc = c.msgs.copy(msgs, off_or_domain, s); if (rc) return rc; }
    HIPCHK(hipEventRecord(tl_ctx->fork, s));
    return BLSMI_OK;
}
// Right after the form's hash_dev: the keys and the infinity flags travel while the messages are hashed; the main stream then waits for the signatures.
int rlc_upload_keys(RlcCall& c, const uint8_t* pks, const uint8_t* inf_flags, int fmt) {
    hipStream_t s = g_stream;
    int rc = upload_points(c.k.pk(), (fmt & FMT_PK_JAC) != 0, pks, c.dp.p, c.n, s);
    if (rc) return rc;
    c.has_inf = inf_flags != nullptr;
    if (inf_flags) HIPCHK(hipMemcpyAsync(c.di.p, inf_flags, c.n, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamWaitEvent(s, tl_ctx->join[1], 0));
    return BLSMI_OK;
}
// a key or a signature that is the all-zero record, or flagged by the caller: a byte per tuple into c.flags, and `any`
void rlc_flag_inputs(RlcCall& c) {
    launch_quiet(KERNEL_OF(k_flag_zero_records), nblocks(c.n), g_stream, c.dp.p, c.k.pk_bytes / 4, c.ds.p, c.k.sig_bytes / 4, c.inf(), c.flags.p, c.any.p, c.n);
}
// r_i times the G1 point of tuple i -- src: the hash points (g2pubs; they stay for the fallback) or the keys (g1pubs) -- into `scaled`.  A scaled
// point at infinity is flagged like an input: into flag_bytes (c.flags, or bytes of the form's own where the inputs' flags must stay), and `any`.
void rlc_scale_g1(RlcCall& c, const u8* src, u8* scaled, u8* sinf, u8* flag_bytes) {
    hipStream_t s = g_stream;
    launch(group_kernels(1).mul_u64, nblocks(c.n), s, src, c.dr.p, scaled, sinf, c.n);
    prof_mark(nullptr);
    launch_quiet(KERNEL_OF(k_flag_zero_records), nblocks(c.n), s, scaled, 24, nullptr, 0, sinf, flag_bytes, c.any.p, c.n);
}
// sum r_i sig_i and its Miller loop on the side stream, beside the tuple side: the kernels and their profile marks go where the context's
// stream points (OnStream); join[0] marks the end (sig_side_start_dev)
int rlc_signature_side(RlcCall& c) {
    hipStream_t st = tl_ctx->aux[0];
    HIPCHK(hipStreamWaitEvent(st, tl_ctx->fork, 0));
    OnStream on(st);
    int rc = rlc_sig_sum(c.k.sig(), c.ds.as<u8>(), c.dr.as<u64>(), c.n, c.sum.as<u8>(), c.sflag.as<i32>()); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(&c.sum_inf, c.sflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    return sig_side_start_dev(c.kind, c.sum.as<u8>(), c.ss);
}
// The end of a combined check, d_prod being the tuple side's product: `any` comes back, the signature side starts (sig_side == false: it
// has, in an earlier attempt of this call), aggregate_tail waits for the side stream and synchronises the main one.  Then c.held() is valid.
int rlc_check_total(RlcCall& c, const i32* d_prod, bool sig_side = true) {
    HIPCHK(hipMemcpyAsync(&c.bad, c.any.p, sizeof(int), hipMemcpyDeviceToHost, g_stream));
    if (sig_side) { int rc = rlc_signature_side(c); if (rc) return rc; }
    return aggregate_tail(d_prod, c.ss, &c.verdict);
}
// the per-tuple verdicts of verify_batch for all n tuples, from the inputs on the device and their hash points d_h
int rlc_fallback_all(RlcCall& c, const u8* d_h, const VerifyRoute& vr) {
    DBuf f; HIPCHK(f.alloc(sizeof(i32) * 12 * NL * c.n));
    return verify_pair_stage(c.kind, d_h, c.dp.p, c.ds.p, c.inf(), c.dok.p, f.as<i32>(), c.n, g_stream, vr);
}
// the verdict bytes back (ok may be null), the end of the call's device work, the bitmap and *combined for the callers that ask
int rlc_finish(RlcCall& c, uint8_t* ok, uint8_t* ok_bitmap, int* combined) {
    if (ok) HIPCHK(hipMemcpyAsync(ok, c.dok.p, c.n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    if (ok_bitmap) pack_bitmap(ok, ok_bitmap, c.n);
    if (combined) *combined = c.held() ? 1 : 0;
    return BLSMI_OK;
}

// One shard on the leased context (tune(): the call's snapshot).  ok: n verdict bytes (host, may be null); d_bitmap_slice as in
// verify_batch_leased; *held = true when the combined check held and every verdict is 1.  r: n nonzero scalars (host).
// Its own: from AGG_POW_MIN g2pubs tuples the hash points stay uncleared and the product is raised to 1 - x (agg_pow_wanted); a message
// that route does not cover sends the tuple side round once more with the cleared points, over the inputs and the signature side that are there.
int rlc_shard(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
              const uint64_t* r, uint8_t* ok, size_t n, int fmt, bool* held, u8* d_bitmap_slice = nullptr) {
    *held = false;
    if (n == 0) return BLSMI_OK;
    const Tuning& t = tune();
    const size_t load = route_load(n);
    const size_t words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    RlcCall c;
    int rc = rlc_begin(c, kind, n, off_or_domain, n); if (rc) return rc;
    DBuf h, scaled, sinf, fr0, fr1, pc;
    HIPCHK(h.alloc((size_t)c.k.h_bytes * n)); HIPCHK(scaled.alloc((size_t)96 * n)); HIPCHK(sinf.alloc(n));
    rc = rlc_upload_start(c, sigs, r, msgs, off_or_domain, fmt); if (rc) return rc;
    bool powc = agg_pow_wanted(kind, n, t);                                // g2pubs from AGG_POW_MIN: uncleared hash points, the product raised to 1 - x
    bool first = true, cleared = !powc;
    // the tuple side: hash, scale, Miller loops, product tree (+ the cofactor power); then the signature side on the side stream; then the tail
    auto combined_check = [&]() -> int {
        const AggregateRoute ar = aggregate_route(kind, n, false, !powc, t, load);
        HIPCHK(fr0.alloc(sizeof(i32) * words * ar.records)); HIPCHK(fr1.alloc(sizeof(i32) * words * ((ar.records + 1) / 2)));
        HIPCHK(hipMemsetAsync(c.any.p, 0, sizeof(int), s));
        int rc = hash_dev(kind, c.msgs.m.p, c.msgs.off.p, h.as<u8>(), n, s, ar.hash, !powc, powc ? c.any.as<int>() : nullptr);   // bad bit 1: a hash point the uncleared path does not cover
        if (rc) return rc;
        cleared = !powc;
        if (first) { rc = rlc_upload_keys(c, pks, inf_flags, fmt); if (rc) return rc; }
        rlc_flag_inputs(c);
        rlc_scale_g1(c, kind == 0 ? h.as<u8>() : c.dp.as<u8>(), scaled.as<u8>(), sinf.as<u8>(), c.flags.as<u8>());
        launch_miller1(scaled.as<u8>(), kind == 0 ? c.dp.as<u8>() : h.as<u8>(), fr0.as<i32>(), n, s, ar, nullptr);
        const i32* prod = prod_tree(fr0.as<i32>(), ar.records, fr1.as<i32>(), fr0.as<i32>(), s);
        HIPCHK(hipGetLastError());
        if (powc) { HIPCHK(pc.alloc(sizeof(i32) * words)); rc = aggregate_pow_c(prod, pc.as<i32>()); if (rc) return rc; prod = pc.as<i32>(); }
        const bool sig_side = first;
        first = false;
        return rlc_check_total(c, prod, sig_side);
    };
    rc = combined_check();
    if (rc) return rc;
    if (!(c.bad & 1) && (c.bad & 2)) { powc = false; rc = combined_check(); if (rc) return rc; }   // an uncovered hash point: once more with the cleared points
    *held = c.held();
    if (*held) HIPCHK(hipMemsetAsync(c.dok.p, 1, n, s));
    else {
        // the per-tuple verdicts of verify_batch, from the inputs on the device (the hash again where h holds uncleared points)
        const VerifyRoute vr = verify_route(kind, n, false, false, t, load);
        if (!cleared) { rc = hash_dev(kind, c.msgs.m.p, c.msgs.off.p, h.as<u8>(), n, s, vr.hash); if (rc) return rc; }
        rc = rlc_fallback_all(c, h.as<u8>(), vr); if (rc) return rc;
    }
    if (d_bitmap_slice) launch_quiet(KERNEL_OF(k_pack_bitmap), nblocks((n + 7) / 8), s, c.dok.p, d_bitmap_slice, n);   // (a split call: the bitmap comes together on the devices)
    return rlc_finish(c, ok, nullptr, nullptr);
}
// The host entry points.  scalars (may be null: drawn here) are checked for zeros first; below the call's rlc_min the per-tuple path runs
// directly.  A split call (plan_shards) runs one combined check per shard, each with its own fallback; the bitmap comes together as in
// verify_batch_direct.  *combined (may be null) = 1 when every verdict came from a combined check that held.
int verify_batch_rlc_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                          const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, int fmt = 0) {
    if (combined) *combined = 0;
    int rc = rlc_check_args(msgs && off_or_domain && pks && sigs, scalars, n);
    if (rc || n == 0) return rc;
    { std::lock_guard<std::mutex> lk(g_mu); rc = ensure_init_default(); if (rc) return rc; }
    const Tuning t = tuning_now();                                         // the call's options, once: every shard routes by this snapshot
    if (n < t.rlc_min) return verify_batch_direct(kind, msgs, off_or_domain, pks, sigs, inf_flags, ok, ok_bitmap, n, fmt);
    const Kind k = kind_of(kind);
    const ShardPlan plan = plan_shards(n, 64);
    RlcHostScratch hs;
    rc = rlc_scalars_and_ok(hs, scalars, ok, !ok && ok_bitmap && plan.nshards == 1, n);   // (a split call packs its bitmap on the devices)
    if (rc) return rc;
    std::unique_ptr<bool[]> held(new bool[plan.nshards]());
    std::unique_lock<std::mutex> coll_lk(g_coll_mu, std::defer_lock);
    const size_t bm = (n + 7) / 8;
    if (plan.nshards > 1 && ok_bitmap) { coll_lk.lock(); int rc = coll_reserve_all(bm, true); if (rc) return rc; }
    rc = run_shards(plan, [&](int sh, size_t lo, size_t hi) -> int {
        tl_ctx->tune = t;
        const size_t m = hi - lo;
        std::vector<uint64_t> off_sub;
        const uint8_t* mp; const uint64_t* op;
        if (kind == 2) { mp = msgs + 32 * lo; op = off_or_domain; }
        else {
            off_sub.resize(m + 1);
            for (size_t i = 0; i <= m; i++) off_sub[i] = off_or_domain[lo + i] - off_or_domain[lo];
            mp = msgs + off_or_domain[lo]; op = off_sub.data();
        }
        u8* slice = (plan.nshards > 1 && ok_bitmap) ? reinterpret_cast<u8*>(tl_ctx->dev->coll.p) + lo / 8 : nullptr;
        return rlc_shard(kind, mp, op, pks + rec_bytes(k.pk_bytes, fmt & FMT_PK_JAC) * lo, sigs + rec_bytes(k.sig_bytes, fmt & FMT_SIG_JAC) * lo,
                         inf_flags ? inf_flags + lo : nullptr, scalars + lo, ok ? ok + lo : nullptr, m, fmt, &held[sh], slice);
    });
    if (rc) return rc;
    if (ok_bitmap) {
        if (plan.nshards == 1) pack_bitmap(ok, ok_bitmap, n);
        else {
            rc = allreduce_bitmap(bm);
            if (rc) return rc;
            HIPCHK(hipSetDevice(g_dev[0].id));
            HIPCHK(hipMemcpyAsync(ok_bitmap, g_dev[0].coll.p, bm, hipMemcpyDeviceToHost, g_dev[0].coll_stream));
            HIPCHK(hipStreamSynchronize(g_dev[0].coll_stream));
        }
    }
    bool all = true;
    for (int i = 0; i < plan.nshards; i++) all = all && held[i];
    if (combined) *combined = all ? 1 : 0;
    return BLSMI_OK;
}
}  // namespace
#define JACP(p) reinterpret_cast<const uint8_t*>(p)
BLSMI_API int blsmi_g2pubs_verify_batch_rlc(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                                             const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_host(0, msgs, off, pks, sigs, inf_flags, scalars, ok, ok_bitmap, n, combined);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                                             const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_host(1, msgs, off, pks, sigs, inf_flags, scalars, ok, ok_bitmap, n, combined);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc(const uint8_t* msgs32, const uint8_t domain[8], const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                                                         const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    if (n && !domain) return BLSMI_E_ARG;
    return verify_batch_rlc_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), pks, sigs, inf_flags, scalars, ok, ok_bitmap, n, combined);
}
BLSMI_API int blsmi_g2pubs_verify_batch_rlc_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t* sigs, const uint64_t* scalars,
                                                 uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_host(0, msgs, off, JACP(pks), JACP(sigs), nullptr, scalars, ok, ok_bitmap, n, combined, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t* sigs, const uint64_t* scalars,
                                                 uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_host(1, msgs, off, JACP(pks), JACP(sigs), nullptr, scalars, ok, ok_bitmap, n, combined, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc_jac(const uint8_t* msgs32, const uint8_t domain[8], const uint64_t* pks, const uint64_t* sigs, const uint64_t* scalars,
                                                             uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    if (n && !domain) return BLSMI_E_ARG;
    return verify_batch_rlc_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), JACP(pks), JACP(sigs), nullptr, scalars, ok, ok_bitmap, n, combined, FMT_JAC);
}

// ---- grouped randomised batch verification (blsmi 0.11; include/blsmi.h "grouped") -------------------------------------------------------
// The combined check of rlc_shard for batches whose n tuples share d messages: tuple i is (msgs[msg_idx[i]], pk_i, sig_i), and bilinearity
// lets the tuples of one message share one pairing --
//     g1pubs: e(G1gen, sum_i r_i sig_i) == prod_g e(sum_{i in g} r_i pk_i, H(m_g))      g2pubs: e(sum_i r_i sig_i, G2gen) == prod_g e(H(m_g), sum_{i in g} r_i pk_i)
// d' hashes and d' Miller loops for the d' messages some tuple refers to, instead of n of each.  The keys' side is the weighted segmented
// sum (segsum_dev with scalars: k_g?_segsum_chunk_u64, no inversion per tuple) over the host plan of group_plan.h; the signature side is
// rlc_shard's (rlc_sig_sum on the side stream, sig_side_start_dev, aggregate_tail).  One lease, one device, no request combiner; "rlc_min"
// is not consulted: calling this form is the caller's choice of the combined path.  When the check fails, or a point at infinity meets it
// (an input, a group's sum, the signatures' sum), the per-tuple verdicts of verify_batch come from the buffers on the device, the d' hash
// points gathered per tuple (k_gather_records).
namespace {
// The host plan of a grouped call (group_plan.h) and the messages some tuple refers to, compacted in table order into cm with the offsets
// coff (kind 2: 32 bytes each, no offsets) -- an entry nobody refers to is never hashed.  BLSMI_E_ARG: some msg_idx[i] >= d (d == 0
// included), or offsets that decrease.
int grouped_plan_and_messages(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, size_t d, const uint32_t* msg_idx, size_t n, blsmi_route::GroupPlan& gp,
                              std::vector<uint64_t>& coff, std::vector<uint8_t>& cm) {
    try {
        if (!blsmi_route::group_plan(msg_idx, n, d, gp)) return BLSMI_E_ARG;
        const size_t dg = gp.msg_of.size();
        if (kind == 2) {
            cm.resize(32 * dg);
            for (size_t g = 0; g < dg; g++) memcpy(cm.data() + 32 * g, msgs + (size_t)32 * gp.msg_of[g], 32);
        } else {
            coff.assign(dg + 1, 0);
            for (size_t g = 0; g < dg; g++) {
                const uint64_t a = off_or_domain[gp.msg_of[g]], b = off_or_domain[gp.msg_of[g] + 1];
                if (b < a) return BLSMI_E_ARG;
                coff[g + 1] = coff[g] + (b - a);
            }
            cm.resize((size_t)coff[dg]);
            for (size_t g = 0; g < dg; g++) if (coff[g + 1] > coff[g]) memcpy(cm.data() + coff[g], msgs + off_or_domain[gp.msg_of[g]], (size_t)(coff[g + 1] - coff[g]));
        }
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    return BLSMI_OK;
}
int verify_batch_rlc_grouped_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                  const uint8_t* inf_flags, const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, int fmt = 0) {
    if (combined) *combined = 0;
    int rc = rlc_check_args(msgs && off_or_domain && msg_idx && pks && sigs && n <= 0xffffffffull, scalars, n);   // (n: the permutation is the 32-bit idx of the segmented sum)
    if (rc || n == 0) return rc;
    blsmi_route::GroupPlan gp;
    std::vector<uint64_t> coff;
    std::vector<uint8_t> cm;
    rc = grouped_plan_and_messages(kind, msgs, off_or_domain, d, msg_idx, n, gp, coff, cm); if (rc) return rc;
    RlcHostScratch hs;
    rc = rlc_scalars_and_ok(hs, scalars, ok, !ok && ok_bitmap, n); if (rc) return rc;
    { std::lock_guard<std::mutex> lk(g_mu); rc = ensure_init_default(); if (rc) return rc; }
    CtxLease lease;
    if (lease.rc) return lease.rc;
    const Tuning& t = tune();
    const size_t dg = gp.msg_of.size();
    const size_t words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    RlcCall c;
    rc = rlc_begin(c, kind, n, kind == 2 ? (const void*)off_or_domain : (const void*)coff.data(), dg);   // the d' messages some tuple refers to
    if (rc) return rc;
    const Kind& k = c.k;
    SegPlan plan;
    segsum_plan(gp.seg_off.data(), dg, segsum_chunk_of(n), plan, 64, 1);
    const AggregateRoute ar = aggregate_route(kind, dg, false, true, t, route_load(dg));   // the layout an aggregate of d' records takes; always cleared hash points
    DBuf dx, h, agg, ainf, gflags, fr0, fr1;
    HIPCHK(dx.alloc(sizeof(uint32_t) * n)); HIPCHK(h.alloc((size_t)k.h_bytes * dg)); HIPCHK(agg.alloc((size_t)k.pk_bytes * dg)); HIPCHK(ainf.alloc(dg)); HIPCHK(gflags.alloc(dg));
    HIPCHK(fr0.alloc(sizeof(i32) * words * ar.records)); HIPCHK(fr1.alloc(sizeof(i32) * words * ((ar.records + 1) / 2)));
    rc = rlc_upload_start(c, sigs, scalars, cm.data(), kind == 2 ? (const void*)off_or_domain : (const void*)coff.data(), fmt); if (rc) return rc;
    HIPCHK(hipMemsetAsync(c.any.p, 0, sizeof(int), s));
    rc = hash_dev(kind, c.msgs.m.p, c.msgs.off.p, h.as<u8>(), dg, s, ar.hash);
    if (rc) return rc;
    rc = rlc_upload_keys(c, pks, inf_flags, fmt); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dx.p, gp.perm.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));   // the plan's permutation, behind the keys
    rlc_flag_inputs(c);
    // sum_{i in g} r_i pk_i for every group; a sum at infinity is flagged like an input.  On s, the context's main stream: segsum_dev names
    // k_g?_segsum_chunk_u64 in the profile only there (profile marks are events on that stream), and tests/test_gpu_rlc_grouped.py looks
    // for the name -- a move of the sums to aux[1] must point the context's stream at it for the stretch (OnStream, as rlc_signature_side)
    rc = segsum_dev(k.pk(), false, c.dp.p, nullptr, n, dx.as<u32>(), plan, agg.as<u8>(), ainf.as<u8>(), 1, s, c.dr.as<u64>());
    if (rc) return rc;
    launch_quiet(KERNEL_OF(k_flag_zero_records), nblocks(dg), s, agg.p, k.pk_bytes / 4, nullptr, 0, ainf.p, gflags.p, c.any.p, dg);
    // d' Miller loops, one per message, and their product
    launch_miller1(kind == 0 ? h.as<u8>() : agg.as<u8>(), kind == 0 ? agg.as<u8>() : h.as<u8>(), fr0.as<i32>(), dg, s, ar, nullptr);
    const i32* prod = prod_tree(fr0.as<i32>(), ar.records, fr1.as<i32>(), fr0.as<i32>(), s);
    HIPCHK(hipGetLastError());
    rc = rlc_check_total(c, prod); if (rc) return rc;
    if (c.held()) HIPCHK(hipMemsetAsync(c.dok.p, 1, n, s));
    else {
        // the per-tuple verdicts of verify_batch: every tuple's hash point from its group's, then the pair stage of a batch of n
        DBuf hfull, dgo;
        HIPCHK(hfull.alloc((size_t)k.h_bytes * n)); HIPCHK(dgo.alloc(sizeof(uint32_t) * n));
        HIPCHK(hipMemcpyAsync(dgo.p, gp.group_of.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
        const u32 hw = (u32)(k.h_bytes / 4);
        launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)hw * n), s, h.p, dgo.p, hfull.p, hw, n);
        rc = rlc_fallback_all(c, hfull.as<u8>(), verify_route(kind, n, false, false, t, route_load(n))); if (rc) return rc;
    }
    return rlc_finish(c, ok, ok_bitmap, combined);
}
}  // namespace
BLSMI_API int blsmi_g2pubs_verify_batch_rlc_grouped(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                                    const uint8_t* inf_flags, const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_grouped_host(0, msgs, msg_off, d, msg_idx, pks, sigs, inf_flags, scalars, ok, ok_bitmap, n, combined);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc_grouped(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                                    const uint8_t* inf_flags, const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_grouped_host(1, msgs, msg_off, d, msg_idx, pks, sigs, inf_flags, scalars, ok, ok_bitmap, n, combined);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped(const uint8_t* msgs32, const uint8_t domain[8], size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                                                const uint8_t* inf_flags, const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_grouped_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), d, msg_idx, pks, sigs, inf_flags, scalars, ok, ok_bitmap, n, combined);
}
BLSMI_API int blsmi_g2pubs_verify_batch_rlc_grouped_jac(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint64_t* pks, const uint64_t* sigs,
                                                        const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_grouped_host(0, msgs, msg_off, d, msg_idx, reinterpret_cast<const uint8_t*>(pks), reinterpret_cast<const uint8_t*>(sigs), nullptr, scalars, ok, ok_bitmap, n, combined, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc_grouped_jac(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint64_t* pks, const uint64_t* sigs,
                                                        const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_grouped_host(1, msgs, msg_off, d, msg_idx, reinterpret_cast<const uint8_t*>(pks), reinterpret_cast<const uint8_t*>(sigs), nullptr, scalars, ok, ok_bitmap, n, combined, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_jac(const uint8_t* msgs32, const uint8_t domain[8], size_t d, const uint32_t* msg_idx, const uint64_t* pks, const uint64_t* sigs,
                                                                    const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined) {
    return verify_batch_rlc_grouped_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), d, msg_idx, reinterpret_cast<const uint8_t*>(pks), reinterpret_cast<const uint8_t*>(sigs), nullptr, scalars,
                                         ok, ok_bitmap, n, combined, FMT_JAC);
}

// ---- randomised batch verification that finds the bad tuples by blocks (blsmi 0.12; include/blsmi.h "locate") -----------------------------
// rlc_shard's combined check with the batch cut into B contiguous blocks of `block` tuples (locate_plan.h).  The tuple side's Miller values
// are multiplied block by block first (k_fq12_seg_prod_row over the blocks' record borders) and the B block values KEPT; the product tree
// then runs over those for the total, which is checked as in rlc_shard.  When the total holds and nothing is flagged every verdict is 1.
// Otherwise one pairing equation per block --
//     g2pubs: e(S_b, G2gen) == prod_{i in b} e(r_i H(m_i), pk_i)        g1pubs: e(G1gen, S_b) == prod_{i in b} e(r_i pk_i, H(m_i))        S_b = sum_{i in b} r_i sig_i
// -- decides which blocks hold: the S_b by the weighted segmented sum, B Miller loops for (-S_b, G2gen) / (-G1gen, S_b), each times its block
// value (k_fq12_mul_pairs_row), B final exponentiations, the comparison with one.  A block whose weights are its own tuples' r_i is wrong
// with probability at most 2^-64, as the whole batch is.  A block with a flagged tuple, or whose S_b is at infinity, counts as failing
// whatever its equation says.  The tuples of the failing blocks, and only those, are gathered into dense buffers and get verify_batch's
// per-tuple verdicts.  One lease, one device, no request combiner, "rlc_min" not consulted.  The hash points are always cleared here, also
// where rlc_shard raises the product to 1 - x instead (agg_pow_wanted): the block values then need no exponentiation each and the
// per-tuple stage reads the hash points that are there (DESIGN 3l has what that costs the call that holds).
namespace {
// Stages 4 and 5, when the total failed: S_b for every block, the B signature-side Miller values in the layout a Pairing call of B tuples
// takes, each times its block value, the final exponentiations in the layout a pairing product of B items takes, one byte per block; then
// `pos`, the positions of the failing blocks' tuples.  sflags: the flag bytes of the scaled points.  Synchronises the main stream.
int locate_failing_positions(RlcCall& c, const blsmi_route::LocatePlan& lp, const i32* bval, const u8* sflags, std::vector<uint32_t>& pos) {
    const Kind& k = c.k;
    const size_t n = c.n, B = lp.blocks(), words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    SegPlan splan;
    std::vector<uint8_t> fail;
    try { segsum_plan(lp.tup_off.data(), B, segsum_chunk_of(n), splan, 64, 1); fail.resize(B); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t bload = route_load(B);
    const Layout fe = pprod_fe_layout(B, bload);
    DBuf sb, sbinf, g1, g2, bbad, fs, prod, vals, one, dfail;
    HIPCHK(sb.alloc((size_t)k.sig_bytes * B)); HIPCHK(sbinf.alloc(B)); HIPCHK(g1.alloc((size_t)96 * B)); HIPCHK(g2.alloc((size_t)192 * B)); HIPCHK(bbad.alloc(B));
    HIPCHK(fs.alloc(sizeof(i32) * words * B)); HIPCHK(prod.alloc(fe == Layout::wave ? 576 * B : sizeof(i32) * words * B)); HIPCHK(vals.alloc(576 * B));
    HIPCHK(one.alloc(B)); HIPCHK(dfail.alloc(B));
    int rc = segsum_dev(k.sig(), false, c.ds.p, nullptr, n, nullptr, splan, sb.as<u8>(), sbinf.as<u8>(), 1, s, c.dr.as<u64>());
    if (rc) return rc;
    launch(KERNEL_OF(k_locate_sig_pairs), nblocks(B), s, c.kind == 0 ? 0 : 1, sb.p, sbinf.p, g_gens.g1, g_gens.g2, g1.p, g2.p, bbad.p, B);
    launch_miller_tuples(g1.as<u8>(), g2.as<u8>(), fs.as<i32>(), B, s, pairing_layout(0, B, tune(), bload));
    launch(KERNEL_OF(k_fq12_mul_pairs_row), tuple_blocks(Layout::row, B), s, bval, fs.p, fe == Layout::wave ? (i32*)nullptr : prod.as<i32>(), fe == Layout::wave ? prod.as<u64>() : (u64*)nullptr, B);
    final_exp_values(fe, prod.p, vals.as<u64>(), one.p, B, s);
    launch(KERNEL_OF(k_locate_block_fail), tuple_blocks(Layout::row, B), s, c.flags.p, sflags, n, lp.block, bbad.p, one.p, dfail.p, B);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(fail.data(), dfail.p, B, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    try { blsmi_route::locate_positions(lp, fail.data(), pos); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    return BLSMI_OK;
}
// Stage 6: the tuples at `pos` (those of the failing blocks), gathered into dense buffers with their hash points h; verify_batch's pair stage
// routed by their count; the verdicts back into c.dok.  hpos (null: pos): a second index list, as long as pos, where the hash point of
// pos[r] is h[hpos[r]] -- a grouped call keeps one hash point per message.
int locate_recheck(RlcCall& c, const DBuf& h, const std::vector<uint32_t>& pos, const std::vector<uint32_t>* hpos = nullptr) {
    const Kind& k = c.k;
    const size_t nre = pos.size(), words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    DBuf dpos, dhpos, hd, pd, sd, id, okd, f;
    HIPCHK(dpos.alloc(sizeof(uint32_t) * nre)); HIPCHK(hd.alloc((size_t)k.h_bytes * nre)); HIPCHK(pd.alloc((size_t)k.pk_bytes * nre)); HIPCHK(sd.alloc((size_t)k.sig_bytes * nre));
    HIPCHK(id.alloc(nre)); HIPCHK(okd.alloc(nre)); HIPCHK(f.alloc(sizeof(i32) * words * nre));
    HIPCHK(hipMemcpyAsync(dpos.p, pos.data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s));
    if (hpos) { HIPCHK(dhpos.alloc(sizeof(uint32_t) * nre)); HIPCHK(hipMemcpyAsync(dhpos.p, hpos->data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s)); }
    auto gather_by = [&](const DBuf& from, DBuf& to, size_t bytes, const DBuf& by) {
        const u32 q = (u32)(bytes / 16);
        launch_quiet(KERNEL_OF(k_gather_records16), nblocks((size_t)q * nre), s, from.p, by.p, to.p, q, nre);
    };
    auto gather = [&](const DBuf& from, DBuf& to, size_t bytes) { gather_by(from, to, bytes, dpos); };
    prof_mark(KERNEL_OF(k_gather_records16).name);                     // one segment: the gathers
    gather_by(h, hd, k.h_bytes, hpos ? dhpos : dpos); gather(c.dp, pd, k.pk_bytes); gather(c.ds, sd, k.sig_bytes);
    if (c.has_inf) launch_quiet(KERNEL_OF(k_gather_bytes), nblocks(nre), s, c.di.p, dpos.p, id.p, nre);
    prof_mark(nullptr);
    const VerifyRoute vr = verify_route(c.kind, nre, false, false, tune(), route_load(nre));
    int rc = verify_pair_stage(c.kind, hd.as<u8>(), pd.p, sd.p, c.has_inf ? id.p : nullptr, okd.p, f.as<i32>(), nre, s, vr);
    if (rc) return rc;
    launch(KERNEL_OF(k_scatter_bytes), nblocks(nre), s, okd.p, dpos.p, c.dok.p, nre);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
int verify_batch_rlc_locate_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                                 const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked, int fmt = 0) {
    if (combined) *combined = 0;
    if (rechecked) *rechecked = 0;
    if (!blsmi_route::locate_block_valid(block)) return BLSMI_E_ARG;
    int rc = rlc_check_args(msgs && off_or_domain && pks && sigs && n <= 0xffffffffull, scalars, n);   // (n: the positions of the failing blocks are 32-bit indices)
    if (rc || n == 0) return rc;
    RlcHostScratch hs;
    rc = rlc_scalars_and_ok(hs, scalars, ok, !ok && ok_bitmap, n); if (rc) return rc;
    { std::lock_guard<std::mutex> lk(g_mu); rc = ensure_init_default(); if (rc) return rc; }
    CtxLease lease;
    if (lease.rc) return lease.rc;
    const Tuning& t = tune();
    const size_t load = route_load(n);
    const size_t words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    const AggregateRoute ar = aggregate_route(kind, n, false, true, t, load);   // always cleared hash points
    const size_t nrec = ar.records;
    blsmi_route::LocatePlan lp;
    SegPlan bplan;
    try {
        blsmi_route::locate_plan(n, block ? block : blsmi_route::locate_auto_block(n), nrec != n, lp);
        pprod_plan(lp.rec_off.data(), lp.blocks(), bplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t B = lp.blocks(), half = (B + 1) / 2;
    RlcCall c;
    rc = rlc_begin(c, kind, n, off_or_domain, n); if (rc) return rc;
    const Kind& k = c.k;
    DBuf h, scaled, sinf, sflags, fr, bval, t0, t1, bblob;
    HIPCHK(h.alloc((size_t)k.h_bytes * n)); HIPCHK(scaled.alloc((size_t)96 * n)); HIPCHK(sinf.alloc(n)); HIPCHK(sflags.alloc(n));
    HIPCHK(fr.alloc(sizeof(i32) * words * nrec)); HIPCHK(bval.alloc(sizeof(i32) * words * B)); HIPCHK(t0.alloc(sizeof(i32) * words * half)); HIPCHK(t1.alloc(sizeof(i32) * words * half));
    HIPCHK(bblob.alloc(bplan.blob.size()));
    // stage 1, as rlc_shard: the uploads, the hash, the flags, r_i H_i / r_i pk_i (flagged into bytes of their own: the inputs' flags stay for the block checks), the Miller loops
    rc = rlc_upload_start(c, sigs, scalars, msgs, off_or_domain, fmt); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(bblob.p, bplan.blob.data(), bplan.blob.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c.any.p, 0, sizeof(int), s));
    rc = hash_dev(kind, c.msgs.m.p, c.msgs.off.p, h.as<u8>(), n, s, ar.hash);
    if (rc) return rc;
    rc = rlc_upload_keys(c, pks, inf_flags, fmt); if (rc) return rc;
    rlc_flag_inputs(c);
    rlc_scale_g1(c, kind == 0 ? h.as<u8>() : c.dp.as<u8>(), scaled.as<u8>(), sinf.as<u8>(), sflags.as<u8>());
    launch_miller1(scaled.as<u8>(), kind == 0 ? c.dp.as<u8>() : h.as<u8>(), fr.as<i32>(), n, s, ar, nullptr);
    // stage 2: the block values, then the tree over them (its levels alternate between t0 and t1; the block values stay)
    prof_mark(KERNEL_OF(k_fq12_seg_prod_row).name);                        // one segment: the passes of seg_prod_dev
    rc = seg_prod_dev(fr.as<i32>(), nrec, nullptr, bplan, bblob.as<u8>(), bval.as<i32>(), nullptr, s);
    if (rc) return rc;
    prof_mark(nullptr);
    const i32* total = prod_tree(bval.as<i32>(), B, t0.as<i32>(), t1.as<i32>(), s);
    HIPCHK(hipGetLastError());
    // stage 3: sum r_i sig_i and its Miller loop on the side stream, the tail
    rc = rlc_check_total(c, total); if (rc) return rc;
    HIPCHK(hipMemsetAsync(c.dok.p, 1, n, s));
    std::vector<uint32_t> pos;
    if (!c.held()) { rc = locate_failing_positions(c, lp, bval.as<i32>(), sflags.as<u8>(), pos); if (rc) return rc; }
    const size_t nre = pos.size();
    if (nre) { rc = locate_recheck(c, h, pos); if (rc) return rc; }
    rc = rlc_finish(c, ok, ok_bitmap, combined);
    if (rechecked && !rc) *rechecked = nre;
    return rc;
}
}  // namespace
BLSMI_API int blsmi_g2pubs_verify_batch_rlc_locate(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                                                   const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    return verify_batch_rlc_locate_host(0, msgs, off, pks, sigs, inf_flags, scalars, block, ok, ok_bitmap, n, combined, rechecked);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc_locate(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                                                   const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    return verify_batch_rlc_locate_host(1, msgs, off, pks, sigs, inf_flags, scalars, block, ok, ok_bitmap, n, combined, rechecked);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc_locate(const uint8_t* msgs32, const uint8_t domain[8], const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags,
                                                               const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    return verify_batch_rlc_locate_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), pks, sigs, inf_flags, scalars, block, ok, ok_bitmap, n, combined, rechecked);
}
BLSMI_API int blsmi_g2pubs_verify_batch_rlc_locate_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t* sigs, const uint64_t* scalars, size_t block,
                                                       uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    return verify_batch_rlc_locate_host(0, msgs, off, JACP(pks), JACP(sigs), nullptr, scalars, block, ok, ok_bitmap, n, combined, rechecked, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc_locate_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t* sigs, const uint64_t* scalars, size_t block,
                                                       uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    return verify_batch_rlc_locate_host(1, msgs, off, JACP(pks), JACP(sigs), nullptr, scalars, block, ok, ok_bitmap, n, combined, rechecked, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc_locate_jac(const uint8_t* msgs32, const uint8_t domain[8], const uint64_t* pks, const uint64_t* sigs, const uint64_t* scalars, size_t block,
                                                                   uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    return verify_batch_rlc_locate_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), JACP(pks), JACP(sigs), nullptr, scalars, block, ok, ok_bitmap, n, combined, rechecked, FMT_JAC);
}
// ---- grouped randomised batch verification that finds the bad tuples by cells (blsmi 0.13; include/blsmi.h "grouped_locate") -------------
// The grouped form's combined check with every group cut into cells of at most `block` tuples (cell_plan.h), and BOTH sides summed per
// cell from the start: K_c = sum_{i in c} r_i pk_i and S_c = sum_{i in c} r_i sig_i, two weighted segmented sums over one plan (idx = the
// group plan's permutation, the cells as segments), the keys on the main stream, the signatures on the side stream in place of
// rlc_sig_sum's MSM.  sum_i r_i sig_i is then the plain sum of the C values S_c, and the tuple side's total the product of the C Miller
// values of (H_g(c), K_c) / (K_c, H_g(c)), which are KEPT.  When the total fails, or something is flagged, one equation per cell decides --
//     g2pubs: e(S_c, G2gen) == e(H_g(c), K_c)        g1pubs: e(G1gen, S_c) == e(K_c, H_g(c))
// -- from what is on the device: C Miller loops for the signature side, each times its kept cell value, C final exponentiations.  Nothing
// is scaled again.  The tuples of the failing cells go through locate_recheck.  One value per cell in every layout: the cells' Miller loops
// take the route of a Pairing call of C tuples (launch_miller_tuples), not an aggregate's, whose quad and pair layouts leave one value per
// two consecutive records and would merge neighbouring cells.  One lease, one device, no request combiner, "rlc_min" not consulted.
namespace {
// what the driver keeps per cell on the device: the two sums with their flags, and the Miller values of the tuple side
struct CellBufs { DBuf dx, kc, kinf, kflag, sc, scinf, cval; };
// S_c for every cell, their sum into c.sum / c.sflag and its Miller loop, on the side stream (as rlc_signature_side; dx, the permutation,
// is on the device by the time `fork` says so)
int cells_signature_side(RlcCall& c, const SegPlan& plan, CellBufs& b) {
    hipStream_t st = tl_ctx->aux[0];
    const size_t C = plan.m;
    HIPCHK(hipStreamWaitEvent(st, tl_ctx->fork, 0));
    OnStream on(st);
    int rc = segsum_dev(c.k.sig(), false, c.ds.p, nullptr, c.n, b.dx.as<u32>(), plan, b.sc.as<u8>(), b.scinf.as<u8>(), 1, st, c.dr.as<u64>());
    if (rc) return rc;
    rc = sum_dev(c.k.sig(), b.sc.as<u8>(), b.scinf.as<u8>(), C, c.sum.as<u8>(), c.sflag.as<i32>(), st, false);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(&c.sum_inf, c.sflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    return sig_side_start_dev(c.kind, c.sum.as<u8>(), c.ss);
}
// When the total failed: the C signature-side Miller values of (-S_c, G2gen) / (-G1gen, S_c), each times its cell value, the final
// exponentiations, one byte per cell (k_locate_cell_fail); then the tuples of the failing cells.  Synchronises the main stream.
int cells_failing_positions(RlcCall& c, const blsmi_route::GroupPlan& gp, const blsmi_route::CellPlan& cp, CellBufs& b, std::vector<uint32_t>& pos, std::vector<uint32_t>& grp) {
    const size_t C = cp.cells(), words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    std::vector<uint8_t> fail;
    try { fail.resize(C); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t cload = route_load(C);
    const Layout fe = pprod_fe_layout(C, cload);
    DBuf g1, g2, sbad, fs, prod, vals, one, dfail, doff;
    HIPCHK(g1.alloc((size_t)96 * C)); HIPCHK(g2.alloc((size_t)192 * C)); HIPCHK(sbad.alloc(C)); HIPCHK(fs.alloc(sizeof(i32) * words * C));
    HIPCHK(prod.alloc(fe == Layout::wave ? 576 * C : sizeof(i32) * words * C)); HIPCHK(vals.alloc(576 * C)); HIPCHK(one.alloc(C)); HIPCHK(dfail.alloc(C));
    HIPCHK(doff.alloc(sizeof(uint64_t) * (C + 1)));
    HIPCHK(hipMemcpyAsync(doff.p, cp.cell_off.data(), sizeof(uint64_t) * (C + 1), hipMemcpyHostToDevice, s));
    launch(KERNEL_OF(k_locate_sig_pairs), nblocks(C), s, c.kind == 0 ? 0 : 1, b.sc.p, b.scinf.p, g_gens.g1, g_gens.g2, g1.p, g2.p, sbad.p, C);
    launch_miller_tuples(g1.as<u8>(), g2.as<u8>(), fs.as<i32>(), C, s, pairing_layout(0, C, tune(), cload));
    launch(KERNEL_OF(k_fq12_mul_pairs_row), tuple_blocks(Layout::row, C), s, b.cval.p, fs.p, fe == Layout::wave ? (i32*)nullptr : prod.as<i32>(), fe == Layout::wave ? prod.as<u64>() : (u64*)nullptr, C);
    final_exp_values(fe, prod.p, vals.as<u64>(), one.p, C, s);
    launch(KERNEL_OF(k_locate_cell_fail), tuple_blocks(Layout::row, C), s, c.flags.p, nullptr, b.dx.p, doff.p, b.kflag.p, sbad.p, one.p, dfail.p, c.n, C);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(fail.data(), dfail.p, C, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    try { blsmi_route::cell_positions(gp, cp, fail.data(), pos, grp); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    return BLSMI_OK;
}
int verify_batch_rlc_grouped_locate_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                         const uint8_t* inf_flags, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked, int fmt = 0) {
    if (combined) *combined = 0;
    if (rechecked) *rechecked = 0;
    int rc = rlc_check_args(msgs && off_or_domain && msg_idx && pks && sigs && n <= 0xffffffffull, scalars, n);   // (n: the permutation and the positions are 32-bit indices)
    if (rc || n == 0) return rc;
    blsmi_route::GroupPlan gp;
    blsmi_route::CellPlan cp;
    std::vector<uint64_t> coff;
    std::vector<uint8_t> cm;
    rc = grouped_plan_and_messages(kind, msgs, off_or_domain, d, msg_idx, n, gp, coff, cm); if (rc) return rc;
    RlcHostScratch hs;
    rc = rlc_scalars_and_ok(hs, scalars, ok, !ok && ok_bitmap, n); if (rc) return rc;
    { std::lock_guard<std::mutex> lk(g_mu); rc = ensure_init_default(); if (rc) return rc; }
    CtxLease lease;
    if (lease.rc) return lease.rc;
    const Tuning& t = tune();
    SegPlan plan;
    try {
        blsmi_route::cell_plan(gp, block ? block : blsmi_route::locate_auto_block(n), cp);
        segsum_plan(cp.cell_off.data(), cp.cells(), segsum_chunk_of(n), plan, 64, 1);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t dg = gp.msg_of.size(), C = cp.cells(), half = (C + 1) / 2;
    const size_t words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    RlcCall c;
    rc = rlc_begin(c, kind, n, kind == 2 ? (const void*)off_or_domain : (const void*)coff.data(), dg);   // the d' messages some tuple refers to
    if (rc) return rc;
    const Kind& k = c.k;
    const HashRoute hr = aggregate_route(kind, dg, false, true, t, route_load(dg)).hash;   // the hash of the grouped form; always cleared hash points
    CellBufs b;
    DBuf h, hc, dcg, t0, t1;
    HIPCHK(b.dx.alloc(sizeof(uint32_t) * n)); HIPCHK(b.kc.alloc((size_t)k.pk_bytes * C)); HIPCHK(b.kinf.alloc(C)); HIPCHK(b.kflag.alloc(C));
    HIPCHK(b.sc.alloc((size_t)k.sig_bytes * C)); HIPCHK(b.scinf.alloc(C)); HIPCHK(b.cval.alloc(sizeof(i32) * words * C));
    HIPCHK(h.alloc((size_t)k.h_bytes * dg)); HIPCHK(hc.alloc((size_t)k.h_bytes * C)); HIPCHK(dcg.alloc(sizeof(uint32_t) * C));
    HIPCHK(t0.alloc(sizeof(i32) * words * half)); HIPCHK(t1.alloc(sizeof(i32) * words * half));
    // the uploads, the hash and the flags as in the grouped form; the permutation goes ahead of the keys and `fork` is recorded again behind it,
    // since the side stream's sums read it
    rc = rlc_upload_start(c, sigs, scalars, cm.data(), kind == 2 ? (const void*)off_or_domain : (const void*)coff.data(), fmt); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(b.dx.p, gp.perm.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dcg.p, cp.group_of.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(tl_ctx->fork, s));
    HIPCHK(hipMemsetAsync(c.any.p, 0, sizeof(int), s));
    rc = hash_dev(kind, c.msgs.m.p, c.msgs.off.p, h.as<u8>(), dg, s, hr);
    if (rc) return rc;
    rc = rlc_upload_keys(c, pks, inf_flags, fmt); if (rc) return rc;
    rlc_flag_inputs(c);
    // K_c for every cell (on the main stream: the profile names k_g?_segsum_chunk_u64 there); a sum at infinity is flagged per cell
    rc = segsum_dev(k.pk(), false, c.dp.p, nullptr, n, b.dx.as<u32>(), plan, b.kc.as<u8>(), b.kinf.as<u8>(), 1, s, c.dr.as<u64>());
    if (rc) return rc;
    launch_quiet(KERNEL_OF(k_flag_zero_records), nblocks(C), s, b.kc.p, k.pk_bytes / 4, nullptr, 0, b.kinf.p, b.kflag.p, c.any.p, C);
    // every cell its group's hash point, C Miller loops with one value each, the values kept; the tree over them gives the total
    const u32 hw = (u32)(k.h_bytes / 4);
    launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)hw * C), s, h.p, dcg.p, hc.p, hw, C);
    launch_miller_tuples(kind == 0 ? hc.as<u8>() : b.kc.as<u8>(), kind == 0 ? b.kc.as<u8>() : hc.as<u8>(), b.cval.as<i32>(), C, s, pairing_layout(0, C, t, route_load(C)));
    prof_mark(nullptr);
    const i32* total = prod_tree(b.cval.as<i32>(), C, t0.as<i32>(), t1.as<i32>(), s);
    HIPCHK(hipGetLastError());
    rc = cells_signature_side(c, plan, b); if (rc) return rc;
    rc = rlc_check_total(c, total, false); if (rc) return rc;
    HIPCHK(hipMemsetAsync(c.dok.p, 1, n, s));
    std::vector<uint32_t> pos, grp;
    if (!c.held()) { rc = cells_failing_positions(c, gp, cp, b, pos, grp); if (rc) return rc; }
    const size_t nre = pos.size();
    if (nre) { rc = locate_recheck(c, h, pos, &grp); if (rc) return rc; }
    rc = rlc_finish(c, ok, ok_bitmap, combined);
    if (rechecked && !rc) *rechecked = nre;
    return rc;
}
}  // namespace
#define GLOC(kind, m, o) return verify_batch_rlc_grouped_locate_host(kind, m, o, d, msg_idx, pks, sigs, inf_flags, scalars, block, ok, ok_bitmap, n, combined, rechecked)
#define GLOCJ(kind, m, o) return verify_batch_rlc_grouped_locate_host(kind, m, o, d, msg_idx, JACP(pks), JACP(sigs), nullptr, scalars, block, ok, ok_bitmap, n, combined, rechecked, FMT_JAC)
BLSMI_API int blsmi_g2pubs_verify_batch_rlc_grouped_locate(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                                           const uint8_t* inf_flags, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    GLOC(0, msgs, msg_off);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc_grouped_locate(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                                           const uint8_t* inf_flags, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    GLOC(1, msgs, msg_off);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate(const uint8_t* msgs32, const uint8_t domain[8], size_t d, const uint32_t* msg_idx, const uint8_t* pks, const uint8_t* sigs,
                                                                       const uint8_t* inf_flags, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    GLOC(2, msgs32, reinterpret_cast<const uint64_t*>(domain));
}
BLSMI_API int blsmi_g2pubs_verify_batch_rlc_grouped_locate_jac(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint64_t* pks, const uint64_t* sigs,
                                                               const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    GLOCJ(0, msgs, msg_off);
}
BLSMI_API int blsmi_g1pubs_verify_batch_rlc_grouped_locate_jac(const uint8_t* msgs, const uint64_t* msg_off, size_t d, const uint32_t* msg_idx, const uint64_t* pks, const uint64_t* sigs,
                                                               const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    GLOCJ(1, msgs, msg_off);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_rlc_grouped_locate_jac(const uint8_t* msgs32, const uint8_t domain[8], size_t d, const uint32_t* msg_idx, const uint64_t* pks, const uint64_t* sigs,
                                                                           const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int* combined, size_t* rechecked) {
    GLOCJ(2, msgs32, reinterpret_cast<const uint64_t*>(domain));
}
#undef GLOC
#undef GLOCJ

// ---- committee aggregates, randomised (blsmi 0.16; include/blsmi.h "committee aggregates, randomised") --------------------------------
// The batches of VerifyAggregateCommon of blsmi 0.9 (verify_host.inc: agg_common_batch_dev) under the grouped form's ONE equation: item j is
// (sig_j, committee j of the registry, table[msg_idx[j]]), and with apk_j the committee's sum
//     g1pubs: e(G1gen, sum_j r_j sig_j) == prod_g e(sum_{j in g} r_j apk_j, H(m_g))      g2pubs: e(sum_j r_j sig_j, G2gen) == prod_g e(H(m_g), sum_{j in g} r_j apk_j)
// The m committee sums are one unweighted segmented sum over the registry (bad_code 1), on aux[1] beside the hash, written where the other
// forms upload one key per tuple: c.dp, their flags (infinity, the empty committee, a bad index) in c.di.  From there c.dp holds m keys and
// the stages of the grouped form run as they stand.  Two things are this driver's own.  Both weighted sums take the pass 1 the options
// choose (GroupKernels::segsum_chunk_u64_opt: G2 a lane pair per ladder, k_g2_segsum_chunk_u64_pair) -- the sizes are hundreds to a few
// thousand points, where one-lane ladders leave most SIMDs idle, and for g2pubs every Miller loop waits for the key side's.  And the
// signature side is the weighted segmented sum over ONE segment [0, m), so that it runs that same pass 1; from RLC_MSM_BUCKET_MIN items
// rlc_sig_sum's bucket route stays.  When the check fails, or anything is flagged, the m Verify()s of 0.9 run from what is on the device
// (k_gather_records of the hash points per item, rlc_fallback_all): the verdicts are those of *_verify_aggregate_common*_batch.
// One lease, one device, no request combiner, "rlc_min" not consulted.
namespace {
// Where the driver finds its inputs, everything on the leased device: the nh messages that are hashed, the registry and the committees'
// indices (null: the positions).  On the host: which hashed message group g of the plan takes (null: g itself) and which item j takes.
struct AggRlcIn {
    const void* d_msgs; const void* d_off_or_domain; size_t nh;
    const void* d_pks; bool pks_jac; size_t npk; const u32* d_idx;
    const uint32_t* h_of_group; const uint32_t* h_of_item;
};
// sum_j r_j sig_j into c.sum / c.sflag and its Miller loop, on the side stream (as rlc_signature_side); `one`: the plan of the one segment
int agg_rlc_signature_side(RlcCall& c, const SegPlan& one) {
    hipStream_t st = tl_ctx->aux[0];
    HIPCHK(hipStreamWaitEvent(st, tl_ctx->fork, 0));
    OnStream on(st);
    int rc;
    if (c.n >= RLC_MSM_BUCKET_MIN) rc = rlc_sig_sum(c.k.sig(), c.ds.as<u8>(), c.dr.as<u64>(), c.n, c.sum.as<u8>(), c.sflag.as<i32>());
    else {
        HIPCHK(hipMemsetAsync(c.sflag.p, 0, sizeof(i32), st));             // (the segmented sum's flag is the word's low byte)
        rc = segsum_dev(c.k.sig(), false, c.ds.p, nullptr, c.n, nullptr, one, c.sum.as<u8>(), c.sflag.as<u8>(), 1, st, c.dr.as<u64>(), &c.k.sig().segsum_chunk_u64_opt);
    }
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(&c.sum_inf, c.sflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    return sig_side_start_dev(c.kind, c.sum.as<u8>(), c.ss);
}
// The call from the point where its inputs are on the device or on their way on the main stream: c.ds the m signatures, c.dr the scalars,
// and what `in` names.  cplan: the committees' chunk plan; gp: the group plan of the m items.  Leaves the verdicts in c.dok, synchronised
// up to the fallback's kernels; c.held() is valid.
int agg_common_rlc_dev(RlcCall& c, const AggRlcIn& in, const SegPlan& cplan, const blsmi_route::GroupPlan& gp) {
    const Kind& k = c.k;
    const int kind = c.kind;
    const Tuning& t = tune();
    const size_t m = c.n, dg = gp.msg_of.size(), words = (size_t)12 * NL;
    hipStream_t s = g_stream, side = tl_ctx->aux[1];
    SegPlan gplan, splan;
    const uint64_t whole[2] = {0, m};
    try {
        segsum_plan(gp.seg_off.data(), dg, segsum_chunk_of(m), gplan, 64, 1);
        if (m < RLC_MSM_BUCKET_MIN) segsum_plan(whole, 1, segsum_chunk_of(m), splan, 64, 1);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t load = route_load(dg);
    const AggregateRoute ar = aggregate_route(kind, dg, false, true, t, load);   // the layout an aggregate of d' records takes; always cleared hash points
    const HashRoute hr = in.nh == dg ? ar.hash : aggregate_route(kind, in.nh, false, true, t, load).hash;
    const u32 hw = (u32)(k.h_bytes / 4);
    DBuf dx, h, hg, dhg, agg, ainf, gflags, fr0, fr1;
    HIPCHK(dx.alloc(sizeof(uint32_t) * m)); HIPCHK(h.alloc((size_t)k.h_bytes * in.nh)); HIPCHK(agg.alloc((size_t)k.pk_bytes * dg)); HIPCHK(ainf.alloc(dg)); HIPCHK(gflags.alloc(dg));
    HIPCHK(fr0.alloc(sizeof(i32) * words * ar.records)); HIPCHK(fr1.alloc(sizeof(i32) * words * ((ar.records + 1) / 2)));
    HIPCHK(hipEventRecord(tl_ctx->fork, s));                               // the inputs are complete here: both side streams start behind it
    // apk_j for every item on aux[1], while the messages are hashed; join[1] marks their arrival
    HIPCHK(hipStreamWaitEvent(side, tl_ctx->fork, 0));
    int rc = segsum_dev(k.pk(), in.pks_jac, in.d_pks, nullptr, in.npk, in.d_idx, cplan, c.dp.as<u8>(), c.di.as<u8>(), 1, side);
    if (rc) return rc;
    HIPCHK(hipEventRecord(tl_ctx->join[1], side));
    c.has_inf = true;                                                      // c.di: a committee that is empty, sums to infinity or holds a bad index
    HIPCHK(hipMemsetAsync(c.any.p, 0, sizeof(int), s));
    HIPCHK(hipMemcpyAsync(dx.p, gp.perm.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, s));
    rc = hash_dev(kind, in.d_msgs, in.d_off_or_domain, h.as<u8>(), in.nh, s, hr);
    if (rc) return rc;
    const u8* hgp = h.as<u8>();                                            // one hash point per group, in group order
    if (in.h_of_group) {
        HIPCHK(hg.alloc((size_t)k.h_bytes * dg)); HIPCHK(dhg.alloc(sizeof(uint32_t) * dg));
        HIPCHK(hipMemcpyAsync(dhg.p, in.h_of_group, sizeof(uint32_t) * dg, hipMemcpyHostToDevice, s));
        launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)hw * dg), s, h.p, dhg.p, hg.p, hw, dg);
        hgp = hg.as<u8>();
    }
    HIPCHK(hipStreamWaitEvent(s, tl_ctx->join[1], 0));
    rlc_flag_inputs(c);
    // sum_{j in g} r_j apk_j for every group, on the main stream (the profile names the pass 1 there); a sum at infinity is flagged like an input
    rc = segsum_dev(k.pk(), false, c.dp.p, nullptr, m, dx.as<u32>(), gplan, agg.as<u8>(), ainf.as<u8>(), 1, s, c.dr.as<u64>(), &k.pk().segsum_chunk_u64_opt);
    if (rc) return rc;
    launch_quiet(KERNEL_OF(k_flag_zero_records), nblocks(dg), s, agg.p, k.pk_bytes / 4, nullptr, 0, ainf.p, gflags.p, c.any.p, dg);
    launch_miller1(kind == 0 ? hgp : agg.as<u8>(), kind == 0 ? agg.as<u8>() : hgp, fr0.as<i32>(), dg, s, ar, nullptr);
    const i32* prod = prod_tree(fr0.as<i32>(), ar.records, fr1.as<i32>(), fr0.as<i32>(), s);
    HIPCHK(hipGetLastError());
    rc = agg_rlc_signature_side(c, splan); if (rc) return rc;
    rc = rlc_check_total(c, prod, false); if (rc) return rc;
    if (c.held()) { HIPCHK(hipMemsetAsync(c.dok.p, 1, m, s)); return BLSMI_OK; }
    // the m Verify()s of the 0.9 call: every item's hash point from the hashed messages, then the pair stage of a batch of m
    DBuf hfull, dhi;
    HIPCHK(hfull.alloc((size_t)k.h_bytes * m)); HIPCHK(dhi.alloc(sizeof(uint32_t) * m));
    HIPCHK(hipMemcpyAsync(dhi.p, in.h_of_item, sizeof(uint32_t) * m, hipMemcpyHostToDevice, s));
    launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)hw * m), s, h.p, dhi.p, hfull.p, hw, m);
    return rlc_fallback_all(c, hfull.as<u8>(), verify_route(kind, m, false, false, t, route_load(m)));
}
int agg_common_rlc_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, size_t d, const uint32_t* msg_idx, const uint8_t* pks, size_t npk, const uint32_t* idx,
                        const uint64_t* seg_off, const uint8_t* sigs, const uint64_t* scalars, uint8_t* ok, uint8_t* ok_bitmap, size_t m, int* combined, int fmt = 0) {
    if (combined) *combined = 0;
    int rc = rlc_check_args(msgs && off_or_domain && msg_idx && sigs && seg_off && (pks || !npk) && (ok || ok_bitmap) && m <= 0xffffffffull, scalars, m);   // (m: the permutation is the 32-bit idx of the segmented sum)
    if (rc || m == 0) return rc;
    rc = segsum_check(npk, idx, seg_off, m); if (rc) return rc;
    blsmi_route::GroupPlan gp;
    std::vector<uint64_t> coff;
    std::vector<uint8_t> cm;
    rc = grouped_plan_and_messages(kind, msgs, off_or_domain, d, msg_idx, m, gp, coff, cm); if (rc) return rc;
    RlcHostScratch hs;
    rc = rlc_scalars_and_ok(hs, scalars, ok, !ok && ok_bitmap, m); if (rc) return rc;
    { std::lock_guard<std::mutex> lk(g_mu); rc = ensure_init_default(); if (rc) return rc; }
    CtxLease lease;
    if (lease.rc) return lease.rc;
    const size_t dg = gp.msg_of.size(), total = seg_off[m];
    const void* hoff = kind == 2 ? (const void*)off_or_domain : (const void*)coff.data();
    SegPlan cplan;
    try { segsum_plan(seg_off, m, segsum_chunk_of(total), cplan); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    hipStream_t s = g_stream;
    RlcCall c;
    rc = rlc_begin(c, kind, m, hoff, dg); if (rc) return rc;            // (the d' messages some item refers to)
    const bool pj = (fmt & FMT_PK_JAC) != 0;
    const size_t pin = rec_bytes(c.k.pk_bytes, pj);
    DBuf reg, dix;
    HIPCHK(reg.alloc(pin * npk)); HIPCHK(dix.alloc(sizeof(uint32_t) * total));
    // the registry as it is (in-memory records are summed as such: k_g?_segsum_chunk_jac), the indices, the signatures, the scalars, the messages
    if (npk) HIPCHK(hipMemcpyAsync(reg.p, pks, pin * npk, hipMemcpyHostToDevice, s));
    if (idx && total) HIPCHK(hipMemcpyAsync(dix.p, idx, sizeof(uint32_t) * total, hipMemcpyHostToDevice, s));
    rc = upload_points(c.k.sig(), (fmt & FMT_SIG_JAC) != 0, sigs, c.ds.p, m, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c.dr.p, scalars, sizeof(uint64_t) * m, hipMemcpyHostToDevice, s));
    rc = c.msgs.copy(cm.data(), hoff, s); if (rc) return rc;
    const AggRlcIn in{c.msgs.m.p, c.msgs.off.p, dg, reg.p, pj, npk, idx ? dix.as<u32>() : nullptr, nullptr, gp.group_of.data()};
    rc = agg_common_rlc_dev(c, in, cplan, gp); if (rc) return rc;
    return rlc_finish(c, ok, ok_bitmap, combined);
}
// the _dev forms: every buffer on one of the library's devices; seg_off and msg_idx come back once for the two plans; every table entry is hashed
template <int KIND>
int agg_common_rlc_dev_api(const void* d_msgs, const void* d_off_or_domain, size_t d, const void* d_msg_idx, const void* d_pks, size_t npk, const void* d_idx, const void* d_seg_off,
                           const void* d_sigs, const uint64_t* scalars, void* d_ok, size_t m, int* combined, void* stream) {
    if (combined) *combined = 0;
    int rc = rlc_check_args(d_msgs && d_off_or_domain && d_msg_idx && d_seg_off && d_sigs && d_ok && (d_pks || !npk) && m <= 0xffffffffull, scalars, m);
    if (rc || m == 0) return rc;
    RlcHostScratch hs;
    uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    hipStream_t s = g_stream;
    std::vector<uint64_t> off;
    std::vector<uint32_t> mi;
    try { mi.resize(m); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    HIPCHK(hipMemcpyAsync(mi.data(), d_msg_idx, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, s));
    rc = segsum_fetch_offsets(d_seg_off, m, off); if (rc) return rc;       // (synchronises: msg_idx is here as well)
    blsmi_route::GroupPlan gp;
    SegPlan cplan;
    try {
        if (!blsmi_route::group_plan(mi.data(), m, d, gp)) return BLSMI_E_ARG;
        segsum_plan(off.data(), m, segsum_chunk_of(off[m]), cplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const uint64_t no_msgs[1] = {0};
    RlcCall c;
    rc = rlc_begin(c, KIND, m, no_msgs, 0); if (rc) return rc;             // (the messages stay where the caller has them)
    HIPCHK(hipMemcpyAsync(c.ds.p, d_sigs, (size_t)c.k.sig_bytes * m, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c.dr.p, scalars, sizeof(uint64_t) * m, hipMemcpyHostToDevice, s));
    const AggRlcIn in{d_msgs, d_off_or_domain, d, d_pks, false, npk, (const u32*)d_idx, gp.msg_of.data(), mi.data()};
    rc = agg_common_rlc_dev(c, in, cplan, gp); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(d_ok, c.dok.p, m, hipMemcpyDeviceToDevice, s));
    return rlc_finish(c, nullptr, nullptr, combined);
}
}  // namespace
#define ACR_ARGS size_t d, const uint32_t* msg_idx, const uint8_t* pks, size_t npk, const uint32_t* idx, const uint64_t* seg_off, const uint8_t* sigs, const uint64_t* scalars, \
                 uint8_t* ok, uint8_t* ok_bitmap, size_t m, int* combined
#define ACR_ARGS_JAC size_t d, const uint32_t* msg_idx, const uint64_t* pks, size_t npk, const uint32_t* idx, const uint64_t* seg_off, const uint64_t* sigs, const uint64_t* scalars, \
                     uint8_t* ok, uint8_t* ok_bitmap, size_t m, int* combined
#define ACR_ARGS_DEV size_t d, const void* d_msg_idx, const void* d_pks, size_t npk, const void* d_idx, const void* d_seg_off, const void* d_sigs, const uint64_t* scalars, \
                     void* d_ok, size_t m, int* combined, void* stream
#define ACR(kind, ms, o) return agg_common_rlc_host(kind, ms, o, d, msg_idx, pks, npk, idx, seg_off, sigs, scalars, ok, ok_bitmap, m, combined)
#define ACRJ(kind, ms, o) return agg_common_rlc_host(kind, ms, o, d, msg_idx, JACP(pks), npk, idx, seg_off, JACP(sigs), scalars, ok, ok_bitmap, m, combined, FMT_JAC)
#define ACRD(kind, ms, o) return agg_common_rlc_dev_api<kind>(ms, o, d, d_msg_idx, d_pks, npk, d_idx, d_seg_off, d_sigs, scalars, d_ok, m, combined, stream)
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_batch_rlc(const uint8_t* msgs, const uint64_t* msg_off, ACR_ARGS) { ACR(0, msgs, msg_off); }
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_batch_rlc(const uint8_t* msgs, const uint64_t* msg_off, ACR_ARGS) { ACR(1, msgs, msg_off); }
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc(const uint8_t* msgs32, const uint8_t domain[8], ACR_ARGS) { ACR(2, msgs32, reinterpret_cast<const uint64_t*>(domain)); }
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_batch_rlc_jac(const uint8_t* msgs, const uint64_t* msg_off, ACR_ARGS_JAC) { ACRJ(0, msgs, msg_off); }
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_batch_rlc_jac(const uint8_t* msgs, const uint64_t* msg_off, ACR_ARGS_JAC) { ACRJ(1, msgs, msg_off); }
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_jac(const uint8_t* msgs32, const uint8_t domain[8], ACR_ARGS_JAC) { ACRJ(2, msgs32, reinterpret_cast<const uint64_t*>(domain)); }
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_batch_rlc_dev(const void* d_msgs, const void* d_msg_off, ACR_ARGS_DEV) { ACRD(0, d_msgs, d_msg_off); }
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_batch_rlc_dev(const void* d_msgs, const void* d_msg_off, ACR_ARGS_DEV) { ACRD(1, d_msgs, d_msg_off); }
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_rlc_dev(const void* d_msgs32, const void* d_domain, ACR_ARGS_DEV) { ACRD(2, d_msgs32, d_domain); }
#undef ACR_ARGS
#undef ACR_ARGS_JAC
#undef ACR_ARGS_DEV
#undef ACR
#undef ACRJ
#undef ACRD
#undef JACP

// ---- pairing products, randomised (blsmi 0.17; include/blsmi.h "pairing products, randomised") -------------------------------------------
// The m equations of blsmi_pairing_product_batch under ONE: pair k = (P_k, table[q_idx[k]]) of item j(k), random nonzero 64-bit r_j,
//     every item holds  <=  FE( prod_g Miller( sum_{k in g} r_j(k) P_k, Q_g ) ) == 1        (g: the table entries some pair refers to)
// by bilinearity -- one Miller loop per entry referred to and one final exponentiation instead of np and m.  Stages, on the call's stream:
//   1  the plan (pprod_rlc_plan.h): groups of pairs per entry, split into shared groups and singletons, compacted shared first
//   2  pprod_weighted_sums: k_pprod_rlc_weights, w_k = r_j(k) and the 0.10 flag byte of every pair (P_k infinite / its entry the all-zero
//      record); shared groups: the weighted segmented G1 sum (segsum_dev with scalars); singletons: k_g1_mul_u64_idx, one lane each
//   3  its own: k_pprod_skip over the d' (S_g, Q_g) -- a sum at infinity or an all-zero entry runs its loop on the generators and is left
//      out: the pair(s) contribute 1, as in 0.10, and the call does NOT leave the combined path for it (an item {(P, Q), (-P, Q)} is
//      legitimate) -- and d' Miller loops in the layout a Pairing call of d' tuples takes
//   4  pprod_check_total: seg_prod_dev over one segment, one final exponentiation, is_one
//   5  the equation held: every verdict is 1 (pprod_all_one).  Otherwise pprod_fallback_all: blsmi_pairing_product_batch's own path
//      (pprod_dev) over all m items from what is on the device, every pair's entry gathered from the compacted table (k_gather_records).
// One lease, one device, never in the request combiner; "rlc_min" is not consulted.  Stages 2 and 4 also serve the form of 0.18 below.
namespace {
struct PprodRlcIn {
    const u8* g1;            // np affine records on the device
    bool own_g1;             // the call's own copy (the per-item path overwrites the records of skipped pairs)
    const u8* flags;         // np caller flags on the device, or null
    u8* tab;                 // the compacted table: d' affine records in the plan's group order, the call's own
    const uint64_t* r;       // host: m nonzero scalars
    const uint64_t* seg_off; // host: the items' offsets
    size_t np, m;
};
// What the weighted sums read of a plan, whichever form made it.  A SEGMENT is what gets one sum and one Miller loop -- a compacted group
// of 0.17, a cell of 0.18 -- the multi-pair ones as segments of a permutation of their pairs, the one-pair ones as a list of pairs.
struct PprodSegments { const uint32_t *item_of, *group_of, *perm, *single; const uint64_t* multi_off; size_t multi, nperm, nsingle, extra; };   // multi_off: multi + 1 offsets into perm
// (extra: sums the weighted sums do not make -- room for them behind their own in S and sinf, filled by the driver before the stage that reads them)
// (of a PprodRlcPlan with its seg_off, of a PprodLocatePlan with its cell_off)
template <class Plan> PprodSegments pprod_segments(const Plan& p, const std::vector<uint64_t>& off, size_t extra = 0) { return {p.item_of.data(), p.group_of.data(), p.perm.data(), p.single.data(), off.data(), off.size() - 1, p.perm.size(), p.single.size(), extra}; }
// What one such check keeps for the length of its call, the counterpart of RlcCall.  On the device: the scalars, the pairs' weights and flag
// bytes, the plan's arrays, the segments' sums S with their infinity flags, the total's one-segment plan, product, final exponentiation and
// verdict.  On the host: the two chunk plans, whose blobs the uploads read, and the verdict byte the last copy targets.  The rule written at
// RlcCall holds: the struct stays where it is until the call has synchronised, and a buffer a later stage reads lives here or in the driver's frame.
struct PprodCall {
    PprodRlcIn in{};
    SegPlan splan, oplan;
    Layout fe{};                                                           // of the total's final exponentiation
    DBuf dr, dw, pflag, dgo, dio, dperm, dsingle, S, sinf, oblob, prod, vals, one;
    uint8_t verdict = 0;
};
// The plans, the buffers, the uploads, k_pprod_rlc_weights, and S = sum_{k in segment} w_k P_k for every segment.  nvals: the values the total
// will be the product of (0.17: the groups' Miller values, 0.18: the blocks' products); load: what lays out its final exponentiation.
int pprod_weighted_sums(PprodCall& c, const PprodRlcIn& in, const PprodSegments& g, size_t nvals, size_t load) {
    c.in = in;
    const size_t np = in.np, nsums = g.multi + g.nsingle;
    hipStream_t s = g_stream;
    const uint64_t whole[2] = {0, nvals};
    try { segsum_plan(g.multi_off, g.multi, segsum_chunk_of(g.nperm), c.splan, 64, 1); pprod_plan(whole, 1, c.oplan); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    c.fe = pprod_fe_layout(1, load);
    HIPCHK(c.dr.alloc(sizeof(uint64_t) * in.m)); HIPCHK(c.dw.alloc(sizeof(uint64_t) * np)); HIPCHK(c.pflag.alloc(np)); HIPCHK(c.dgo.alloc(sizeof(uint32_t) * np));
    HIPCHK(c.dio.alloc(sizeof(uint32_t) * np)); HIPCHK(c.dperm.alloc(sizeof(uint32_t) * g.nperm)); HIPCHK(c.dsingle.alloc(sizeof(uint32_t) * g.nsingle));
    HIPCHK(c.S.alloc((size_t)96 * (nsums + g.extra))); HIPCHK(c.sinf.alloc(nsums + g.extra)); HIPCHK(c.oblob.alloc(c.oplan.blob.size()));
    HIPCHK(c.prod.alloc(c.fe == Layout::wave ? 576 : sizeof(i32) * 12 * NL)); HIPCHK(c.vals.alloc(576)); HIPCHK(c.one.alloc(1));
    HIPCHK(hipMemcpyAsync(c.dr.p, in.r, sizeof(uint64_t) * in.m, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c.dio.p, g.item_of, sizeof(uint32_t) * np, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(c.dgo.p, g.group_of, sizeof(uint32_t) * np, hipMemcpyHostToDevice, s));
    if (g.nperm) HIPCHK(hipMemcpyAsync(c.dperm.p, g.perm, sizeof(uint32_t) * g.nperm, hipMemcpyHostToDevice, s));
    if (g.nsingle) HIPCHK(hipMemcpyAsync(c.dsingle.p, g.single, sizeof(uint32_t) * g.nsingle, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c.oblob.p, c.oplan.blob.data(), c.oplan.blob.size(), hipMemcpyHostToDevice, s));
    launch(KERNEL_OF(k_pprod_rlc_weights), nblocks(np), s, in.g1, in.flags, in.tab, c.dgo.p, c.dio.p, c.dr.p, c.dw.p, c.pflag.p, np);
    prof_mark(nullptr);
    // the multi-pair segments' sums into S[0, multi), the one-pair segments' behind them
    int rc = segsum_dev(group_kernels(1), false, in.g1, c.pflag.as<u8>(), np, c.dperm.as<u32>(), c.splan, c.S.as<u8>(), c.sinf.as<u8>(), 1, s, c.dw.as<u64>());
    if (rc || !g.nsingle) return rc;
    launch(KERNEL_OF(k_g1_mul_u64_idx), nblocks(g.nsingle), s, in.g1, c.pflag.p, c.dw.p, c.dsingle.p, c.S.as<u8>() + (size_t)96 * g.multi, c.sinf.as<u8>() + g.multi, g.nsingle);
    prof_mark(nullptr);
    return BLSMI_OK;
}
// The total: the nvals values at src (skip: the ones left out, or null) multiplied as one segment, the final exponentiation, is_one, the byte back.
// The caller has opened the profile segment of the segmented products (0.18 runs the blocks' products in it too).  Synchronises; *held: the equation held.
int pprod_check_total(PprodCall& c, const i32* src, size_t nvals, const u8* skip, bool* held) {
    hipStream_t s = g_stream;
    const bool wave = c.fe == Layout::wave;
    int rc = seg_prod_dev(src, nvals, skip, c.oplan, c.oblob.as<u8>(), wave ? (i32*)nullptr : c.prod.as<i32>(), wave ? c.prod.as<u64>() : (u64*)nullptr, s); if (rc) return rc;
    final_exp_values(c.fe, c.prod.p, c.vals.as<u64>(), c.one.p, 1, s);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&c.verdict, c.one.p, 1, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    *held = c.verdict == 1;
    return BLSMI_OK;
}
// every verdict is 1; sync: nothing follows on the stream
int pprod_all_one(const PprodCall& c, void* d_is_one, bool sync) {
    HIPCHK(hipMemsetAsync(d_is_one, 1, c.in.m, g_stream));
    if (sync) HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// 0.17, stage 5 when the equation failed: the per-item path of 0.10 over all m items, every pair's table entry from the compacted table (an
// all-zero entry's record now holds the generator: bit 1 of the pair's flag byte, written before, leaves the pair out all the same)
int pprod_fallback_all(PprodCall& c, void* d_is_one) {
    const PprodRlcIn& in = c.in;
    const size_t np = in.np;
    hipStream_t s = g_stream;
    SegPlan iplan; try { pprod_plan(in.seg_off, in.m, iplan); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    DBuf a, b; HIPCHK(b.alloc((size_t)192 * np));
    u8* g1 = const_cast<u8*>(in.g1);
    if (!in.own_g1) { HIPCHK(a.alloc((size_t)96 * np)); HIPCHK(hipMemcpyAsync(a.p, in.g1, (size_t)96 * np, hipMemcpyDeviceToDevice, s)); g1 = a.as<u8>(); }
    launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)48 * np), s, in.tab, c.dgo.p, b.p, 48, np);
    return pprod_dev(g1, b.as<u8>(), c.pflag.as<u8>(), np, iplan, nullptr, d_is_one, s);
}
// d_is_one: m verdict bytes on the device.  Synchronises the call's stream.
int pprod_rlc_core(const PprodRlcIn& in, const blsmi_route::PprodRlcPlan& pl, void* d_is_one, bool* held) {
    const size_t dg = pl.groups();
    hipStream_t s = g_stream;
    PprodCall c; DBuf skip, f;
    HIPCHK(skip.alloc(dg)); HIPCHK(f.alloc(sizeof(i32) * 12 * NL * dg));
    int rc = pprod_weighted_sums(c, in, pprod_segments(pl, pl.seg_off), dg, route_load(dg)); if (rc) return rc;   // stage 2
    launch_quiet(KERNEL_OF(k_pprod_skip), nblocks(dg), s, c.S.p, in.tab, c.sinf.p, g_gens.g1, g_gens.g2, skip.p, dg);   // stage 3
    launch_miller_tuples(c.S.as<u8>(), in.tab, f.as<i32>(), dg, s, pairing_layout(0, dg, tune(), route_load(dg)));
    prof_mark(KERNEL_OF(k_fq12_seg_prod_row).name);                        // one segment: the passes of seg_prod_dev
    rc = pprod_check_total(c, f.as<i32>(), dg, skip.as<u8>(), held); if (rc) return rc;   // stage 4
    return *held ? pprod_all_one(c, d_is_one, true) : pprod_fallback_all(c, d_is_one);   // stage 5
}
// ---- pairing products, randomised, that find the bad items by blocks (blsmi 0.18; include/blsmi.h under the same title) --------------------
// The equation above with the m items cut into B contiguous blocks (pprod_locate_plan.h) and the sums taken per CELL -- (block, table entry)
// with a pair of the block referring to the entry -- so that every block has a product of its own,
//     V_b = prod_{c in b} Miller( sum_{k in c} r_j(k) P_k, Q_g(c) ),        total = prod_b V_b,
// all of it there by the time the total is known: a failing call runs no second ladder, no second Miller loop.  Stages, on the call's stream:
//   1  pprod_weighted_sums, the cells as its segments (idx = the plan's permutation), behind the uploads of the cells' slots
//   2  pprod_locate_failing_blocks --
//      k_pprod_cell_route: every cell's sum and its entry's record into dense arrays in block order, the skip rule on the way (one launch
//      where two record gathers, a byte gather and k_pprod_skip would run);
//      C Miller loops in the layout a Pairing call of C tuples takes: one value per cell in every layout;
//      seg_prod_dev over the blocks' slot borders: B block values, KEPT -- as a hand-off buffer, which the total's product reads, and as
//      in-memory records where their final exponentiation (that of a pairing product of B items) runs in the wave layout;
//      pprod_check_total over the B values (a second, one-segment seg_prod_dev), then every verdict is 1: the answer when the total held;
//      it failed: B final exponentiations, B bytes to the host, the failing blocks' items and pairs (pprod_locate_failing)
//   3  pprod_locate_recheck: the failing blocks' G1 records, flag bytes and per-pair table records gathered dense (the entry indices
//      composed on the host), pprod_dev over them, the verdicts scattered over the ones.  The dense copies are the call's own: nothing of
//      the caller's is written, no full copy of the G1 records is made.
// One lease, one device, never in the request combiner; "rlc_min" is not consulted.
// what the driver keeps of the cells, uploaded ahead of the first kernel: the blocks' chunk plan with its blob, every slot's cell and table entry
struct PprodCellBufs { SegPlan bplan; DBuf bblob, dsum, dent; };
// Stage 2.  *held: the total held, and every verdict is 1.  Otherwise ff has the items and pairs of the failing blocks, and the verdict
// array is preset to 1 for the recheck to scatter over.  Synchronises.
int pprod_locate_failing_blocks(PprodCall& c, const blsmi_route::PprodLocatePlan& pl, const PprodCellBufs& b, void* d_is_one, bool* held, blsmi_route::PprodLocateFailing& ff) {
    const size_t C = pl.cells(), B = pl.blocks(), words = (size_t)12 * NL;
    hipStream_t s = g_stream;
    const Layout feb = pprod_fe_layout(B, route_load(B));
    DBuf g1c, g2c, skip, f, bval, bmem, bvals, bone;
    HIPCHK(g1c.alloc((size_t)96 * C)); HIPCHK(g2c.alloc((size_t)192 * C)); HIPCHK(skip.alloc(C)); HIPCHK(f.alloc(sizeof(i32) * words * C));
    HIPCHK(bval.alloc(sizeof(i32) * words * B)); HIPCHK(bmem.alloc(feb == Layout::wave ? 576 * B : 1));
    launch(KERNEL_OF(k_pprod_cell_route), tuple_blocks(Layout::row, C), s, c.S.p, c.sinf.p, c.in.tab, b.dsum.p, b.dent.p, g_gens.g1, g_gens.g2, g1c.p, g2c.p, skip.p, C, pl.entry_of.size());
    launch_miller_tuples(g1c.as<u8>(), g2c.as<u8>(), f.as<i32>(), C, s, pairing_layout(0, C, tune(), route_load(C)));
    prof_mark(KERNEL_OF(k_fq12_seg_prod_row).name);                        // one segment: the passes of both seg_prod_dev
    int rc = seg_prod_dev(f.as<i32>(), C, skip.as<u8>(), b.bplan, b.bblob.as<u8>(), bval.as<i32>(), feb == Layout::wave ? bmem.as<u64>() : (u64*)nullptr, s);
    if (!rc) rc = pprod_check_total(c, bval.as<i32>(), B, nullptr, held);
    if (!rc) rc = pprod_all_one(c, d_is_one, *held);
    if (rc || *held) return rc;
    // which blocks fail: their kept values through the final exponentiation a pairing product of B items takes
    std::vector<uint8_t> fail; try { fail.resize(B); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    HIPCHK(bvals.alloc(576 * B)); HIPCHK(bone.alloc(B));
    final_exp_values(feb, feb == Layout::wave ? bmem.p : bval.p, bvals.as<u64>(), bone.p, B, s);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(fail.data(), bone.p, B, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    try {
        for (uint8_t& x : fail) x = x == 1 ? 0 : 1;
        blsmi_route::pprod_locate_failing(pl, c.in.seg_off, fail.data(), ff);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    return BLSMI_OK;
}
// The end of a recheck, whoever gathered the dense pairs (a, b, fl: npd of them, the call's own; iplan: the dense items over them):
// blsmi_pairing_product_batch's own path, the verdicts okd scattered to d_is_one[d_items[.]].  Synchronises.
int pprod_recheck_dense(u8* a, u8* b, const u8* fl, size_t npd, const SegPlan& iplan, const u32* d_items, void* okd, void* d_is_one) {
    hipStream_t s = g_stream;
    int rc = pprod_dev(a, b, fl, npd, iplan, nullptr, okd, s); if (rc) return rc;
    launch(KERNEL_OF(k_scatter_bytes), nblocks(iplan.m), s, okd, d_items, d_is_one, iplan.m);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError()); HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
// Stage 3: the failing blocks' items, dense, through blsmi_pairing_product_batch's own path; their verdicts back over the ones.  Synchronises.
int pprod_locate_recheck(PprodCall& c, const blsmi_route::PprodLocateFailing& ff, void* d_is_one) {
    const PprodRlcIn& in = c.in;
    const size_t nre = ff.items.size(), npd = ff.pairs.size();
    hipStream_t s = g_stream;
    SegPlan iplan; try { pprod_plan(ff.dense_off.data(), nre, iplan); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    DBuf ditems, dpairs, dents, a, b, fl, okd;
    HIPCHK(ditems.alloc(sizeof(uint32_t) * nre)); HIPCHK(dpairs.alloc(sizeof(uint32_t) * npd)); HIPCHK(dents.alloc(sizeof(uint32_t) * npd));
    HIPCHK(a.alloc((size_t)96 * npd)); HIPCHK(b.alloc((size_t)192 * npd)); HIPCHK(fl.alloc(npd)); HIPCHK(okd.alloc(nre));
    HIPCHK(hipMemcpyAsync(ditems.p, ff.items.data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s));
    if (npd) {
        HIPCHK(hipMemcpyAsync(dpairs.p, ff.pairs.data(), sizeof(uint32_t) * npd, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dents.p, ff.entries.data(), sizeof(uint32_t) * npd, hipMemcpyHostToDevice, s));
        prof_mark(KERNEL_OF(k_gather_records16).name);                     // one segment: the gathers
        if (reinterpret_cast<uintptr_t>(in.g1) & 15) launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)24 * npd), s, in.g1, dpairs.p, a.p, 24, npd);   // (a caller's buffer)
        else launch_quiet(KERNEL_OF(k_gather_records16), nblocks((size_t)6 * npd), s, in.g1, dpairs.p, a.p, 6, npd);
        launch_quiet(KERNEL_OF(k_gather_records16), nblocks((size_t)12 * npd), s, in.tab, dents.p, b.p, 12, npd);
        launch_quiet(KERNEL_OF(k_gather_bytes), nblocks(npd), s, c.pflag.p, dpairs.p, fl.p, npd);
        prof_mark(nullptr);
    }
    return pprod_recheck_dense(a.as<u8>(), b.as<u8>(), fl.as<u8>(), npd, iplan, ditems.as<u32>(), okd.p, d_is_one);
}
// d_is_one: m verdict bytes on the device.  Synchronises.
int pprod_locate_core(const PprodRlcIn& in, const blsmi_route::PprodLocatePlan& pl, void* d_is_one, bool* held, size_t* rechecked) {
    const size_t C = pl.cells();
    hipStream_t s = g_stream;
    *rechecked = 0;
    PprodCall c; PprodCellBufs b;
    blsmi_route::PprodLocateFailing ff;
    try { pprod_plan(pl.slot_off.data(), pl.blocks(), b.bplan); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    HIPCHK(b.dsum.alloc(sizeof(uint32_t) * C)); HIPCHK(b.dent.alloc(sizeof(uint32_t) * C)); HIPCHK(b.bblob.alloc(b.bplan.blob.size()));
    HIPCHK(hipMemcpyAsync(b.dsum.p, pl.sum_of.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(b.dent.p, pl.entry_at.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.bblob.p, b.bplan.blob.data(), b.bplan.blob.size(), hipMemcpyHostToDevice, s));
    int rc = pprod_weighted_sums(c, in, pprod_segments(pl, pl.cell_off), pl.blocks(), route_load(C)); if (rc) return rc;   // stage 1
    rc = pprod_locate_failing_blocks(c, pl, b, d_is_one, held, ff);        // stage 2
    if (rc || *held) return rc;
    if (ff.items.empty()) { HIPCHK(hipStreamSynchronize(s)); return BLSMI_OK; }   // (cannot be: the total is the product of the block values)
    rc = pprod_locate_recheck(c, ff, d_is_one);                            // stage 3
    if (!rc) *rechecked = ff.items.size();
    return rc;
}
// what makes a call of the two functions below the block-locating form of 0.18 (on): the caller's `block` (0: automatic) and where the
// number of rechecked items goes (may be null)
struct PprodLocate { bool on = false; size_t block = 0; size_t* rechecked = nullptr; };
// *combined and the locating form's *rechecked (either may be null): zero when a call begins, the call's own when it succeeds
void pprod_report(int* combined, const PprodLocate& loc, bool held, size_t nre) { if (combined) *combined = held ? 1 : 0; if (loc.rechecked) *loc.rechecked = nre; }
// The plan of the form a call takes, decided once, and that form's driver.
struct PprodPlans {
    bool locate = false;
    blsmi_route::PprodRlcPlan pl; blsmi_route::PprodLocatePlan lp;
    // false: what the plan functions refuse (BLSMI_E_ARG).  split == false: blsmi_debug_pairing_product_batch_rlc_dev_nosplit.  May throw bad_alloc.
    bool build(const uint64_t* seg_off, size_t m, const uint32_t* q_idx, size_t np, size_t nq, bool split, const PprodLocate& loc) {
        locate = loc.on;
        return locate ? blsmi_route::pprod_locate_plan(seg_off, m, q_idx, np, nq, loc.block ? loc.block : blsmi_route::pprod_locate_auto_block(m), lp)
                      : blsmi_route::pprod_rlc_plan(seg_off, m, q_idx, np, nq, pl, split);
    }
    const std::vector<uint32_t>& entry_of() const { return locate ? lp.entry_of : pl.entry_of; }
    // *nre: the items the per-item path saw after the block equations (0.17: none)
    int run(const PprodRlcIn& in, void* d_is_one, bool* held, size_t* nre) const { return locate ? pprod_locate_core(in, lp, d_is_one, held, nre) : pprod_rlc_core(in, pl, d_is_one, held); }
};
int pprod_rlc_host(const uint8_t* g1, const uint8_t* inf_flags, const uint8_t* tab, size_t nq, const uint32_t* q_idx, size_t np, const uint64_t* seg_off, size_t m,
                   const uint64_t* scalars, uint8_t* is_one, int* combined, bool jac, const PprodLocate& loc = {}) {
    pprod_report(combined, loc, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = rlc_check_args(is_one && seg_off && (np == 0 || (g1 && tab)) && (!loc.on || m <= 0xffffffffull), scalars, m);   // (the items of the failing blocks are 32-bit indices)
    if (rc) return rc;
    PprodPlans plans; std::vector<uint8_t> packed;
    const size_t qb = rec_bytes(192, jac);
    try {
        if (!plans.build(seg_off, m, q_idx, np, nq, true, loc)) return BLSMI_E_ARG;
        if (q_idx) {                                                       // only the entries some pair refers to travel, already in group order
            const std::vector<uint32_t>& entry_of = plans.entry_of();
            packed.resize(qb * entry_of.size());
            for (size_t c = 0; c < entry_of.size(); c++) memcpy(packed.data() + qb * c, tab + qb * entry_of[c], qb);
        }
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    if (np == 0) { memset(is_one, 1, m); pprod_report(combined, loc, true, 0); return BLSMI_OK; }
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    const size_t dg = plans.entry_of().size();
    DBuf a, t, fl, dok;
    HIPCHK(a.alloc((size_t)96 * np)); HIPCHK(t.alloc((size_t)192 * dg)); HIPCHK(fl.alloc(np)); HIPCHK(dok.alloc(m));
    rc = upload_points(group_kernels(1), jac, g1, a.p, np, s); if (rc) return rc;
    rc = upload_points(group_kernels(2), jac, q_idx ? packed.data() : tab, t.p, dg, s); if (rc) return rc;
    if (inf_flags && !jac) HIPCHK(hipMemcpyAsync(fl.p, inf_flags, np, hipMemcpyHostToDevice, s));
    bool held = false; size_t nre = 0;
    const PprodRlcIn in{a.as<u8>(), true, (inf_flags && !jac) ? fl.as<u8>() : nullptr, t.as<u8>(), scalars, seg_off, np, m};
    rc = plans.run(in, dok.p, &held, &nre); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(is_one, dok.p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    pprod_report(combined, loc, held, nre);
    return BLSMI_OK;
}
// the _dev forms: seg_off and q_idx come back once for the plans; the table entries referred to are gathered; the caller's buffers stay untouched.
// split == false: every group through the segmented sum (blsmi_debug_pairing_product_batch_rlc_dev_nosplit).
int pprod_rlc_dev_api(const void* d_g1, const void* d_inf_flags, const void* d_tab, size_t nq, const void* d_q_idx, size_t np, const void* d_seg_off, size_t m,
                      const uint64_t* scalars, void* d_is_one, int* combined, void* stream, bool jac, bool split = true, const PprodLocate& loc = {}) {
    pprod_report(combined, loc, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = rlc_check_args(d_is_one && d_seg_off && (np == 0 || (d_g1 && d_tab)) && (d_q_idx || nq == np) && np <= 0xffffffffull && (!loc.on || m <= 0xffffffffull), scalars, m);
    if (rc) return rc;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT_AT(d_is_one);
    UseStream us(stream);
    hipStream_t s = g_stream;
    std::vector<uint64_t> off; std::vector<uint32_t> qi;
    if (d_q_idx && np) {
        try { qi.resize(np); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
        HIPCHK(hipMemcpyAsync(qi.data(), d_q_idx, sizeof(uint32_t) * np, hipMemcpyDeviceToHost, s));
    }
    rc = segsum_fetch_offsets(d_seg_off, m, off); if (rc) return rc;       // (synchronises: q_idx is here as well)
    PprodPlans plans;
    try {
        if (!plans.build(off.data(), m, d_q_idx ? qi.data() : nullptr, np, nq, split, loc)) return BLSMI_E_ARG;
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    bool held = true; size_t nre = 0;
    if (np == 0) { HIPCHK(hipMemsetAsync(d_is_one, 1, m, s)); HIPCHK(hipStreamSynchronize(s)); }
    else {
        const std::vector<uint32_t>& entry_of = plans.entry_of();
        const size_t dg = entry_of.size();
        DBuf a, t, tj, dent;
        HIPCHK(t.alloc((size_t)192 * dg)); HIPCHK(dent.alloc(sizeof(uint32_t) * dg));
        HIPCHK(hipMemcpyAsync(dent.p, entry_of.data(), sizeof(uint32_t) * dg, hipMemcpyHostToDevice, s));
        const u8* g1 = (const u8*)d_g1;
        if (jac) {
            HIPCHK(a.alloc((size_t)96 * np)); HIPCHK(tj.alloc((size_t)288 * dg));
            rc = jac_to_wire_dev(group_kernels(1), d_g1, a.p, nullptr, np, s); if (rc) return rc;
            launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)72 * dg), s, d_tab, dent.p, tj.p, 72, dg);
            rc = jac_to_wire_dev(group_kernels(2), tj.p, t.p, nullptr, dg, s); if (rc) return rc;
            g1 = a.as<u8>();
        } else launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)48 * dg), s, d_tab, dent.p, t.p, 48, dg);
        const PprodRlcIn in{g1, jac, jac ? nullptr : (const u8*)d_inf_flags, t.as<u8>(), scalars, off.data(), np, m};
        rc = plans.run(in, d_is_one, &held, &nre); if (rc) return rc;
    }
    pprod_report(combined, loc, held, nre);
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_pairing_product_batch_rlc(const uint8_t* g1_aff, const uint8_t* inf_flags, const uint8_t* g2_tab, size_t nq, const uint32_t* q_idx, size_t np, const uint64_t* seg_off, size_t m, const uint64_t* scalars, uint8_t* is_one, int* combined) {
    return pprod_rlc_host(g1_aff, inf_flags, g2_tab, nq, q_idx, np, seg_off, m, scalars, is_one, combined, false);
}
BLSMI_API int blsmi_pairing_product_batch_rlc_jac(const uint64_t* g1_jac, const uint64_t* g2_tab_jac, size_t nq, const uint32_t* q_idx, size_t np, const uint64_t* seg_off, size_t m, const uint64_t* scalars, uint8_t* is_one, int* combined) {
    return pprod_rlc_host(reinterpret_cast<const uint8_t*>(g1_jac), nullptr, reinterpret_cast<const uint8_t*>(g2_tab_jac), nq, q_idx, np, seg_off, m, scalars, is_one, combined, true);
}
BLSMI_API int blsmi_pairing_product_batch_rlc_dev(const void* d_g1_aff, const void* d_inf_flags, const void* d_g2_tab, size_t nq, const void* d_q_idx, size_t np, const void* d_seg_off, size_t m, const uint64_t* scalars, void* d_is_one, int* combined, void* stream) {
    return pprod_rlc_dev_api(d_g1_aff, d_inf_flags, d_g2_tab, nq, d_q_idx, np, d_seg_off, m, scalars, d_is_one, combined, stream, false);
}
BLSMI_API int blsmi_pairing_product_batch_rlc_jac_dev(const void* d_g1_jac, const void* d_g2_tab_jac, size_t nq, const void* d_q_idx, size_t np, const void* d_seg_off, size_t m, const uint64_t* scalars, void* d_is_one, int* combined, void* stream) {
    return pprod_rlc_dev_api(d_g1_jac, nullptr, d_g2_tab_jac, nq, d_q_idx, np, d_seg_off, m, scalars, d_is_one, combined, stream, true);
}
// blsmi_pairing_product_batch_rlc_dev with the singleton groups sent through the weighted segmented sum as well: the other side of the
// by-pass's criterion, kept so that tools/pprod_rlc_bench.py can measure it again
BLSMI_API int blsmi_debug_pairing_product_batch_rlc_dev_nosplit(const void* d_g1_aff, const void* d_inf_flags, const void* d_g2_tab, size_t nq, const void* d_q_idx, size_t np, const void* d_seg_off, size_t m, const uint64_t* scalars, void* d_is_one, int* combined, void* stream) {
    return pprod_rlc_dev_api(d_g1_aff, d_inf_flags, d_g2_tab, nq, d_q_idx, np, d_seg_off, m, scalars, d_is_one, combined, stream, false, false);
}
// the block-locating forms (blsmi 0.18): pprod_locate_core in place of pprod_rlc_core
BLSMI_API int blsmi_pairing_product_batch_rlc_locate(const uint8_t* g1_aff, const uint8_t* inf_flags, const uint8_t* g2_tab, size_t nq, const uint32_t* q_idx, size_t np, const uint64_t* seg_off, size_t m, const uint64_t* scalars, size_t block, uint8_t* is_one, int* combined, size_t* rechecked) {
    return pprod_rlc_host(g1_aff, inf_flags, g2_tab, nq, q_idx, np, seg_off, m, scalars, is_one, combined, false, {true, block, rechecked});
}
BLSMI_API int blsmi_pairing_product_batch_rlc_locate_jac(const uint64_t* g1_jac, const uint64_t* g2_tab_jac, size_t nq, const uint32_t* q_idx, size_t np, const uint64_t* seg_off, size_t m, const uint64_t* scalars, size_t block, uint8_t* is_one, int* combined, size_t* rechecked) {
    return pprod_rlc_host(reinterpret_cast<const uint8_t*>(g1_jac), nullptr, reinterpret_cast<const uint8_t*>(g2_tab_jac), nq, q_idx, np, seg_off, m, scalars, is_one, combined, true, {true, block, rechecked});
}
BLSMI_API int blsmi_pairing_product_batch_rlc_locate_dev(const void* d_g1_aff, const void* d_inf_flags, const void* d_g2_tab, size_t nq, const void* d_q_idx, size_t np, const void* d_seg_off, size_t m, const uint64_t* scalars, size_t block, void* d_is_one, int* combined, size_t* rechecked, void* stream) {
    return pprod_rlc_dev_api(d_g1_aff, d_inf_flags, d_g2_tab, nq, d_q_idx, np, d_seg_off, m, scalars, d_is_one, combined, stream, false, true, {true, block, rechecked});
}
BLSMI_API int blsmi_pairing_product_batch_rlc_locate_jac_dev(const void* d_g1_jac, const void* d_g2_tab_jac, size_t nq, const void* d_q_idx, size_t np, const void* d_seg_off, size_t m, const uint64_t* scalars, size_t block, void* d_is_one, int* combined, size_t* rechecked, void* stream) {
    return pprod_rlc_dev_api(d_g1_jac, nullptr, d_g2_tab_jac, nq, d_q_idx, np, d_seg_off, m, scalars, d_is_one, combined, stream, true, true, {true, block, rechecked});
}

// ---- arithmetic mod r: the weighted segmented fold of scalars (blsmi 0.19; include/blsmi.h "scalar-field folds") ---------------------------
// out[s][0] = sum of the weights of segment s, out[s][1 + i] = sum_j w_j vals[j][i] mod r: k_fr_wsum_u64 over a chunk plan -- every chunk
// the rows of one segment that one workgroup folds -- leaves twelve unreduced words per (chunk, column); k_fr_wsum_fold adds a segment's
// chunks and reduces once per output.  Always both launches, whatever the segments' lengths: the result does not depend on the plan.
namespace {
struct FrWsumPlan { size_t cols = 1, ntile = 1; std::vector<uint64_t> ch_lo, seg_ch; std::vector<uint32_t> ch_cnt; };
// Rows per chunk: sixteen steps of the workgroup's R = 256 / min(ncol + 1, 256) rows, doubled while that leaves more than 2^16 chunks.
void fr_wsum_plan(const uint64_t* seg_off, size_t nseg, size_t ncol, FrWsumPlan& p) {
    p.cols = ncol + 1;
    const size_t cw = std::min<size_t>(p.cols, 256);
    p.ntile = (p.cols + cw - 1) / cw;
    uint64_t rows = 256 / cw * 16;
    while (seg_off[nseg] / rows > ((uint64_t)1 << 16) && rows < ((uint64_t)1 << 28)) rows *= 2;
    p.ch_lo.clear(); p.ch_cnt.clear(); p.seg_ch.assign(1, 0);
    for (size_t j = 0; j < nseg; j++) {
        for (uint64_t a = seg_off[j]; a < seg_off[j + 1]; a += rows) { p.ch_lo.push_back(a); p.ch_cnt.push_back((uint32_t)std::min<uint64_t>(rows, seg_off[j + 1] - a)); }
        p.seg_ch.push_back(p.ch_lo.size());
    }
}
// The fold on the device, on s, not synchronised; the plan stays alive until the caller has.  d_w: one weight per row; d_out: nseg * cols scalars.
int fr_wsum_dev(const FrWsumPlan& p, const void* d_vals, size_t ncol, const void* d_w, size_t nseg, void* d_out, hipStream_t s) {
    const size_t nch = p.ch_lo.size(), nout = nseg * p.cols;
    if (nout == 0) return BLSMI_OK;
    DBuf dlo, dcnt, dseg, part;
    HIPCHK(dlo.alloc(sizeof(uint64_t) * nch)); HIPCHK(dcnt.alloc(sizeof(uint32_t) * nch)); HIPCHK(dseg.alloc(sizeof(uint64_t) * (nseg + 1)));
    HIPCHK(part.alloc(sizeof(uint32_t) * 12 * p.cols * nch));
    if (nch) {
        HIPCHK(hipMemcpyAsync(dlo.p, p.ch_lo.data(), sizeof(uint64_t) * nch, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(dcnt.p, p.ch_cnt.data(), sizeof(uint32_t) * nch, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(dseg.p, p.seg_ch.data(), sizeof(uint64_t) * (nseg + 1), hipMemcpyHostToDevice, s));
    const bool mark = tl_ctx && s == tl_ctx->stream;                       // (profile marks are events on the context's main stream)
    if (mark) prof_mark(KERNEL_OF(k_fr_wsum_u64).name);                    // one segment: both passes
    if (nch) launch_quiet_sized(KERNEL_OF(k_fr_wsum_u64), nch * p.ntile, 256, s, d_vals, ncol, d_w, dlo.p, dcnt.p, part.p, nch);
    launch_quiet_sized(KERNEL_OF(k_fr_wsum_fold), (nout + 255) / 256, 256, s, part.p, dseg.p, p.cols, d_out, nout);
    if (mark) prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
// what both forms refuse: a column count or a row count beyond 32 bits (the accumulator's bound is 2^32 rows)
bool fr_wsum_sizes_ok(size_t ncol, uint64_t n) { return ncol <= 0xffffffffull && n <= 0xffffffffull; }
}  // namespace
BLSMI_API int blsmi_fr_wsum_segmented_u64(const uint8_t* vals, size_t ncol, const uint64_t* weights, const uint64_t* seg_off, size_t nseg, uint8_t* out) {
    if (nseg == 0) return BLSMI_OK;
    if (!seg_off || !out || seg_off[0] != 0) return BLSMI_E_ARG;
    for (size_t j = 0; j < nseg; j++) if (seg_off[j + 1] < seg_off[j]) return BLSMI_E_ARG;
    const uint64_t n = seg_off[nseg];
    if (!fr_wsum_sizes_ok(ncol, n) || (n && !weights) || (n && ncol && !vals)) return BLSMI_E_ARG;
    FrWsumPlan plan;
    try { fr_wsum_plan(seg_off, nseg, ncol, plan); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    DBuf dv, dw, dout;
    HIPCHK(dv.alloc((size_t)32 * ncol * n)); HIPCHK(dw.alloc(sizeof(uint64_t) * n)); HIPCHK(dout.alloc((size_t)32 * plan.cols * nseg));
    if (n && ncol) HIPCHK(hipMemcpyAsync(dv.p, vals, (size_t)32 * ncol * n, hipMemcpyHostToDevice, s));
    if (n) HIPCHK(hipMemcpyAsync(dw.p, weights, sizeof(uint64_t) * n, hipMemcpyHostToDevice, s));
    int rc = fr_wsum_dev(plan, dv.p, ncol, dw.p, nseg, dout.p, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)32 * plan.cols * nseg, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
BLSMI_API int blsmi_fr_wsum_segmented_u64_dev(const void* d_vals, size_t ncol, const void* d_weights, const void* d_seg_off, size_t nseg, void* d_out, void* stream) {
    if (nseg == 0) return BLSMI_OK;
    if (!d_seg_off || !d_out || ncol > 0xffffffffull) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    std::vector<uint64_t> off;
    int rc = segsum_fetch_offsets(d_seg_off, nseg, off); if (rc) return rc;
    const uint64_t n = off[nseg];
    if (!fr_wsum_sizes_ok(ncol, n) || (n && !d_weights) || (n && ncol && !d_vals)) return BLSMI_E_ARG;
    FrWsumPlan plan;
    try { fr_wsum_plan(off.data(), nseg, ncol, plan); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    rc = fr_wsum_dev(plan, d_vals, ncol, d_weights, nseg, d_out, g_stream); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}

// ---- Groth16 batches with the public inputs folded in Fr (blsmi 0.19; include/blsmi.h "Groth16") ----------------------------------------
// m proofs of one circuit under the block equations of 0.18.  Item j holds when e(A_j, B_j) e(alpha, -beta) e(L_j, -gamma) e(C_j, -delta) = 1,
// L_j = IC_0 + sum_i a_ji IC_i -- the key's three G2 points are negated once (k_g2_neg_records), no proof point is.  With the weights r_j,
//     sum_j r_j L_j = t IC_0 + sum_i s_i IC_i,        t = sum_j r_j,    s_i = sum_j r_j a_ji mod r        (the sums over a block)
// so that a block needs nin + 1 scalars from the fold above and nin + 2 full-width ladders, whatever its length.  Stages:
//   1  the plan of 0.18 over two pairs per item, (A_j, B_j) and (C_j, -delta): the blocks' singleton cells and delta cells, and two further
//      cells per block appended to it (pprod_locate_append_cells): alpha against -beta, the folded point against -gamma
//   2  pprod_weighted_sums, unchanged, with room for the 2 B sums it does not make
//   3  its own: fr_wsum_dev over the inputs with the blocks as segments; B (nin + 2) ladders over gathered key points (t_b alpha, t_b IC_0,
//      s_bi IC_i: mul_dev_core); the alpha cells copied, the gamma cells by the segmented sum, into those places
//   4  pprod_locate_failing_blocks, unchanged: route, Miller loops, block products, total, final exponentiation; the failing blocks
//   5  groth16_recheck for their items only: inputs mod r (the fold again, a segment per item, weight one), the ladders and the segmented
//      sum for L_j, the four pairs dense (k_groth16_recheck_pairs), pprod_recheck_dense.
// One lease, one device, never in the request combiner.
namespace {
struct Groth16In {
    const u8* vk_g1;         // alpha, IC_0 .. IC_nin: affine, 16-byte aligned
    const u8* g1;            // A_j, C_j interleaved: 2 m affine records, 16-byte aligned
    const u8* tab;           // B_0 .. B_{m - 1}, -delta, -beta, -gamma: the call's own, affine
    const u8* inputs;        // m * nin scalars (not read when nin == 0)
    const uint64_t* r;       // host: m nonzero scalars
    size_t nin, m, block;    // block: resolved, >= 1
};
const uint32_t GROTH16_KEY_ORDER[3] = {2, 0, 1};                           // vk_g2 is beta, gamma, delta; the table's tail is -delta, -beta, -gamma
// records i of src (idx null: the first n) as n dense records of `bytes` bytes (a multiple of 16), whatever src's alignment
void groth16_gather(const void* src, const DBuf& idx, void* dst, size_t bytes, size_t n, hipStream_t s) {
    if (reinterpret_cast<uintptr_t>(src) & 15) launch_quiet(KERNEL_OF(k_gather_records), nblocks(bytes / 4 * n), s, src, idx.p, dst, bytes / 4, n);
    else launch_quiet(KERNEL_OF(k_gather_records16), nblocks(bytes / 16 * n), s, src, idx.p, dst, bytes / 16, n);
}
// Stage 5.  items: the proofs of the failing blocks, ascending.  Synchronises.
int groth16_recheck(const Groth16In& in, const std::vector<uint32_t>& items, void* d_ok) {
    const size_t nre = items.size(), cols = in.nin + 1, nl = nre * cols;
    hipStream_t s = g_stream;
    const GroupKernels& g = group_kernels(1);
    std::vector<uint64_t> ones, roff, loff, ioff; std::vector<uint32_t> lp;
    FrWsumPlan rp; SegPlan lplan, iplan;
    try {
        ones.assign(nre, 1); roff.resize(nre + 1); loff.resize(nre + 1); ioff.resize(nre + 1); lp.resize(nl);
        for (size_t t = 0; t <= nre; t++) { roff[t] = t; loff[t] = t * cols; ioff[t] = 4 * t; }
        for (size_t k = 0; k < nl; k++) lp[k] = (uint32_t)(1 + k % cols);
        fr_wsum_plan(roff.data(), nre, in.nin, rp); segsum_plan(loff.data(), nre, segsum_chunk_of(nl), lplan); pprod_plan(ioff.data(), nre, iplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    DBuf ditems, rows, dones, rout, dlp, lpts, lout, linf, L, Linf, a, b, fl, okd;
    HIPCHK(ditems.alloc(sizeof(uint32_t) * nre)); HIPCHK(rows.alloc((size_t)32 * in.nin * nre)); HIPCHK(dones.alloc(sizeof(uint64_t) * nre)); HIPCHK(rout.alloc((size_t)32 * nl));
    HIPCHK(dlp.alloc(sizeof(uint32_t) * nl)); HIPCHK(lpts.alloc((size_t)96 * nl)); HIPCHK(lout.alloc((size_t)96 * nl)); HIPCHK(linf.alloc(nl));
    HIPCHK(L.alloc((size_t)96 * nre)); HIPCHK(Linf.alloc(nre)); HIPCHK(a.alloc((size_t)96 * 4 * nre)); HIPCHK(b.alloc((size_t)192 * 4 * nre)); HIPCHK(fl.alloc(4 * nre)); HIPCHK(okd.alloc(nre));
    HIPCHK(hipMemcpyAsync(ditems.p, items.data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dones.p, ones.data(), sizeof(uint64_t) * nre, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dlp.p, lp.data(), sizeof(uint32_t) * nl, hipMemcpyHostToDevice, s));
    prof_mark(KERNEL_OF(k_gather_records16).name);                         // one segment: the gathers
    if (in.nin) groth16_gather(in.inputs, ditems, rows.p, (size_t)32 * in.nin, nre, s);
    groth16_gather(in.vk_g1, dlp, lpts.p, 96, nl, s);
    prof_mark(nullptr);
    int rc = fr_wsum_dev(rp, rows.p, in.nin, dones.p, nre, rout.p, s); if (rc) return rc;   // every row: 1, a_1 mod r, .., a_nin mod r
    rc = mul_dev_core(g, lpts.as<u8>(), rout.as<u8>(), lout.as<u8>(), linf.as<u8>(), nl, s); if (rc) return rc;
    rc = segsum_dev(g, false, lout.p, linf.as<u8>(), nl, nullptr, lplan, L.as<u8>(), Linf.as<u8>(), 1, s); if (rc) return rc;
    launch(KERNEL_OF(k_groth16_recheck_pairs), tuple_blocks(Layout::row, 4 * nre), s, in.g1, in.vk_g1, L.p, Linf.p, in.tab, ditems.p, in.m, a.p, b.p, fl.p, nre);
    prof_mark(nullptr);
    return pprod_recheck_dense(a.as<u8>(), b.as<u8>(), fl.as<u8>(), 4 * nre, iplan, ditems.as<u32>(), okd.p, d_ok);
}
// d_ok: m verdict bytes on the device.  Synchronises.
int groth16_core(const Groth16In& in, void* d_ok, bool* held, size_t* rechecked) {
    const size_t m = in.m, nin = in.nin, np = 2 * m, cols = nin + 1;
    hipStream_t s = g_stream;
    const GroupKernels& g = group_kernels(1);
    *rechecked = 0;
    std::vector<uint64_t> seg_off, boff, goff; std::vector<uint32_t> q_idx, lpt, lsc;
    blsmi_route::PprodLocatePlan pl; blsmi_route::PprodLocateFailing ff;
    FrWsumPlan fp; SegPlan gplan;
    PprodCall c; PprodCellBufs b;
    size_t C0 = 0, B = 0, nl = 0;
    try {
        seg_off.resize(m + 1); q_idx.resize(np);
        for (size_t j = 0; j < m; j++) { seg_off[j] = 2 * j; q_idx[2 * j] = (uint32_t)j; q_idx[2 * j + 1] = (uint32_t)m; }
        seg_off[m] = np;
        if (!blsmi_route::pprod_locate_plan(seg_off.data(), m, q_idx.data(), np, m + 1, in.block, pl)) return BLSMI_E_ARG;   // stage 1
        C0 = pl.cells(); B = pl.blocks(); nl = B * (nin + 2);
        const uint32_t further[2] = {(uint32_t)(m + 1), (uint32_t)(m + 2)};
        blsmi_route::pprod_locate_append_cells(pl, further, 2);
        boff.resize(B + 1); goff.resize(B + 1); lpt.resize(nl); lsc.resize(nl);
        for (size_t k = 0; k < B; k++) {
            boff[k] = pl.item_lo(k); goff[k] = k * cols;
            lpt[k] = 0; lsc[k] = (uint32_t)(k * cols);                     // t_b alpha
            for (size_t i = 0; i < cols; i++) { lpt[B + k * cols + i] = (uint32_t)(1 + i); lsc[B + k * cols + i] = (uint32_t)(k * cols + i); }   // t_b IC_0, s_bi IC_i
        }
        boff[B] = m; goff[B] = B * cols;
        fr_wsum_plan(boff.data(), B, nin, fp); segsum_plan(goff.data(), B, segsum_chunk_of(B * cols), gplan); pprod_plan(pl.slot_off.data(), B, b.bplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t C = pl.cells(), dg = pl.entry_of.size();
    DBuf t, dent, fout, dlp, dls, lpts, lscal, lout, linf;
    HIPCHK(t.alloc((size_t)192 * dg)); HIPCHK(dent.alloc(sizeof(uint32_t) * dg));
    HIPCHK(b.dsum.alloc(sizeof(uint32_t) * C)); HIPCHK(b.dent.alloc(sizeof(uint32_t) * C)); HIPCHK(b.bblob.alloc(b.bplan.blob.size()));
    HIPCHK(fout.alloc((size_t)32 * cols * B)); HIPCHK(dlp.alloc(sizeof(uint32_t) * nl)); HIPCHK(dls.alloc(sizeof(uint32_t) * nl));
    HIPCHK(lpts.alloc((size_t)96 * nl)); HIPCHK(lscal.alloc((size_t)32 * nl)); HIPCHK(lout.alloc((size_t)96 * nl)); HIPCHK(linf.alloc(nl));
    HIPCHK(hipMemcpyAsync(dent.p, pl.entry_of.data(), sizeof(uint32_t) * dg, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.dsum.p, pl.sum_of.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(b.dent.p, pl.entry_at.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.bblob.p, b.bplan.blob.data(), b.bplan.blob.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dlp.p, lpt.data(), sizeof(uint32_t) * nl, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dls.p, lsc.data(), sizeof(uint32_t) * nl, hipMemcpyHostToDevice, s));
    launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)48 * dg), s, in.tab, dent.p, t.p, 48, dg);   // the table in the plan's order
    const PprodRlcIn pin{in.g1, false, nullptr, t.as<u8>(), in.r, seg_off.data(), np, m};
    int rc = pprod_weighted_sums(c, pin, pprod_segments(pl, pl.cell_off, 2 * B), B, route_load(C)); if (rc) return rc;   // stage 2
    rc = fr_wsum_dev(fp, in.inputs, nin, c.dr.p, B, fout.p, s); if (rc) return rc;   // stage 3
    groth16_gather(in.vk_g1, dlp, lpts.p, 96, nl, s);
    groth16_gather(fout.p, dls, lscal.p, 32, nl, s);
    rc = mul_dev_core(g, lpts.as<u8>(), lscal.as<u8>(), lout.as<u8>(), linf.as<u8>(), nl, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c.S.as<u8>() + (size_t)96 * C0, lout.p, (size_t)96 * B, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c.sinf.as<u8>() + C0, linf.p, B, hipMemcpyDeviceToDevice, s));
    rc = segsum_dev(g, false, lout.as<u8>() + (size_t)96 * B, linf.as<u8>() + B, B * cols, nullptr, gplan, c.S.as<u8>() + (size_t)96 * (C0 + B), c.sinf.as<u8>() + C0 + B, 1, s);
    if (rc) return rc;
    rc = pprod_locate_failing_blocks(c, pl, b, d_ok, held, ff);             // stage 4
    if (rc || *held) return rc;
    if (ff.items.empty()) { HIPCHK(hipStreamSynchronize(s)); return BLSMI_OK; }   // (cannot be: the total is the product of the block values)
    rc = groth16_recheck(in, ff.items, d_ok);                               // stage 5
    if (!rc) *rechecked = ff.items.size();
    return rc;
}
// What every form checks before any device work; m beyond 2^31 - 1 is refused (the pairs A_j, C_j are 32-bit indices), nin beyond 2^20.
int groth16_check_args(bool pointers_ok, size_t nin, bool inputs_ok, size_t m, const uint64_t* scalars) {
    if (m > 0x7ffffffeull || nin > ((size_t)1 << 20) || !pointers_ok || (nin && !inputs_ok)) return BLSMI_E_ARG;
    return rlc_check_args(true, scalars, m);
}
void groth16_report(int* combined, size_t* rechecked, bool held, size_t nre) { if (combined) *combined = held ? 1 : 0; if (rechecked) *rechecked = nre; }
// -beta, -gamma, -delta behind the B_j: the table's tail from the key's three affine records on the device
int groth16_key_tail(const void* d_vk_g2_aff, u8* d_tab, size_t m, hipStream_t s) {
    DBuf order; HIPCHK(order.alloc(sizeof(GROTH16_KEY_ORDER)));
    HIPCHK(hipMemcpyAsync(order.p, GROTH16_KEY_ORDER, sizeof(GROTH16_KEY_ORDER), hipMemcpyHostToDevice, s));
    launch_quiet(KERNEL_OF(k_g2_neg_records), 1, s, d_vk_g2_aff, order.p, d_tab + (size_t)192 * m, 3);
    return BLSMI_OK;
}
int groth16_host(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t nin, const uint8_t* proof_g1, const uint8_t* proof_g2, const uint8_t* inputs, size_t m,
                 const uint64_t* scalars, size_t block, uint8_t* ok, int* combined, size_t* rechecked, bool jac) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = groth16_check_args(vk_g1 && vk_g2 && proof_g1 && proof_g2 && ok, nin, inputs != nullptr, m, scalars); if (rc) return rc;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    DBuf vk1, vk2, g1, tab, din, dok;
    HIPCHK(vk1.alloc((size_t)96 * (nin + 2))); HIPCHK(vk2.alloc(192 * 3)); HIPCHK(g1.alloc((size_t)96 * 2 * m)); HIPCHK(tab.alloc((size_t)192 * (m + 3)));
    HIPCHK(din.alloc((size_t)32 * nin * m)); HIPCHK(dok.alloc(m));
    rc = upload_points(group_kernels(1), jac, vk_g1, vk1.p, nin + 2, s); if (rc) return rc;
    rc = upload_points(group_kernels(2), jac, vk_g2, vk2.p, 3, s); if (rc) return rc;
    rc = upload_points(group_kernels(1), jac, proof_g1, g1.p, 2 * m, s); if (rc) return rc;
    rc = upload_points(group_kernels(2), jac, proof_g2, tab.p, m, s); if (rc) return rc;
    if (nin) HIPCHK(hipMemcpyAsync(din.p, inputs, (size_t)32 * nin * m, hipMemcpyHostToDevice, s));
    rc = groth16_key_tail(vk2.p, tab.as<u8>(), m, s); if (rc) return rc;
    bool held = false; size_t nre = 0;
    const Groth16In in{vk1.as<u8>(), g1.as<u8>(), tab.as<u8>(), din.as<u8>(), scalars, nin, m, block ? block : blsmi_route::pprod_locate_auto_block(m)};
    rc = groth16_core(in, dok.p, &held, &nre); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ok, dok.p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
// the _dev forms: the B_j and the negated key points go into a table of the call's own; affine records that are 16-byte aligned are read in place
int groth16_dev_api(const void* d_vk_g1, const void* d_vk_g2, size_t nin, const void* d_proof_g1, const void* d_proof_g2, const void* d_inputs, size_t m,
                    const uint64_t* scalars, size_t block, void* d_ok, int* combined, size_t* rechecked, void* stream, bool jac) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = groth16_check_args(d_vk_g1 && d_vk_g2 && d_proof_g1 && d_proof_g2 && d_ok, nin, d_inputs != nullptr, m, scalars); if (rc) return rc;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    hipStream_t s = g_stream;
    DBuf vk1, vk2, g1, tab;
    HIPCHK(tab.alloc((size_t)192 * (m + 3)));
    const u8 *pvk1 = (const u8*)d_vk_g1, *pg1 = (const u8*)d_proof_g1; const void* pvk2 = d_vk_g2;
    // a G1 buffer of the call's own: in-memory records converted, or a caller's affine records that are not 16-byte aligned copied
    auto own_g1 = [&](DBuf& d, const u8*& p, size_t n) -> int {
        if (!jac && (reinterpret_cast<uintptr_t>(p) & 15) == 0) return BLSMI_OK;
        HIPCHK(d.alloc((size_t)96 * n));
        if (jac) { int rc = jac_to_wire_dev(group_kernels(1), p, d.p, nullptr, n, s); if (rc) return rc; }
        else HIPCHK(hipMemcpyAsync(d.p, p, (size_t)96 * n, hipMemcpyDeviceToDevice, s));
        p = d.as<u8>();
        return BLSMI_OK;
    };
    rc = own_g1(vk1, pvk1, nin + 2); if (rc) return rc;
    rc = own_g1(g1, pg1, 2 * m); if (rc) return rc;
    if (jac) {
        HIPCHK(vk2.alloc(192 * 3));
        rc = jac_to_wire_dev(group_kernels(2), d_vk_g2, vk2.p, nullptr, 3, s); if (rc) return rc;
        rc = jac_to_wire_dev(group_kernels(2), d_proof_g2, tab.p, nullptr, m, s); if (rc) return rc;
        pvk2 = vk2.p;
    } else HIPCHK(hipMemcpyAsync(tab.p, d_proof_g2, (size_t)192 * m, hipMemcpyDeviceToDevice, s));
    rc = groth16_key_tail(pvk2, tab.as<u8>(), m, s); if (rc) return rc;
    bool held = false; size_t nre = 0;
    const Groth16In in{pvk1, pg1, tab.as<u8>(), (const u8*)d_inputs, scalars, nin, m, block ? block : blsmi_route::pprod_locate_auto_block(m)};
    rc = groth16_core(in, d_ok, &held, &nre); if (rc) return rc;
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_groth16_verify_batch(const uint8_t* vk_g1, const uint8_t* vk_g2, size_t nin, const uint8_t* proof_g1, const uint8_t* proof_g2, const uint8_t* inputs, size_t m,
                                         const uint64_t* scalars, size_t block, uint8_t* ok, int* combined, size_t* rechecked) {
    return groth16_host(vk_g1, vk_g2, nin, proof_g1, proof_g2, inputs, m, scalars, block, ok, combined, rechecked, false);
}
BLSMI_API int blsmi_groth16_verify_batch_jac(const uint64_t* vk_g1_jac, const uint64_t* vk_g2_jac, size_t nin, const uint64_t* proof_g1_jac, const uint64_t* proof_g2_jac, const uint8_t* inputs, size_t m,
                                             const uint64_t* scalars, size_t block, uint8_t* ok, int* combined, size_t* rechecked) {
    return groth16_host(reinterpret_cast<const uint8_t*>(vk_g1_jac), reinterpret_cast<const uint8_t*>(vk_g2_jac), nin, reinterpret_cast<const uint8_t*>(proof_g1_jac),
                        reinterpret_cast<const uint8_t*>(proof_g2_jac), inputs, m, scalars, block, ok, combined, rechecked, true);
}
BLSMI_API int blsmi_groth16_verify_batch_dev(const void* d_vk_g1, const void* d_vk_g2, size_t nin, const void* d_proof_g1, const void* d_proof_g2, const void* d_inputs, size_t m,
                                             const uint64_t* scalars, size_t block, void* d_ok, int* combined, size_t* rechecked, void* stream) {
    return groth16_dev_api(d_vk_g1, d_vk_g2, nin, d_proof_g1, d_proof_g2, d_inputs, m, scalars, block, d_ok, combined, rechecked, stream, false);
}
BLSMI_API int blsmi_groth16_verify_batch_jac_dev(const void* d_vk_g1_jac, const void* d_vk_g2_jac, size_t nin, const void* d_proof_g1_jac, const void* d_proof_g2_jac, const void* d_inputs, size_t m,
                                                 const uint64_t* scalars, size_t block, void* d_ok, int* combined, size_t* rechecked, void* stream) {
    return groth16_dev_api(d_vk_g1_jac, d_vk_g2_jac, nin, d_proof_g1_jac, d_proof_g2_jac, d_inputs, m, scalars, block, d_ok, combined, rechecked, stream, true);
}

// ---- KZG batches with the values folded in Fr (blsmi 0.20; include/blsmi.h "KZG") -----------------------------------------------------------
// out_j = A_j + [k_j mod r] B_j, a lane per item (k_g1_mul_add_glv, k_kzg.hip): the endomorphism ladder, one mixed addition, one inversion.
namespace {
// a stride of affine G1 records: 0 (one common record) or at least a record, in whole words
bool mul_add_stride_ok(size_t stride) { return stride == 0 || (stride >= 96 && stride % 4 == 0); }
// the bytes n records `stride` apart span
size_t mul_add_span(size_t stride, size_t n) { return stride * (n - 1) + 96; }
// on s, not synchronised
int mul_add_dev_core(const u8* d_a, size_t a_stride, const u8* d_b, size_t b_stride, const u8* d_scalars, u8* d_out, size_t out_stride, u8* d_out_inf, size_t n, hipStream_t s) {
    launch(KERNEL_OF(k_g1_mul_add_glv), nblocks(n), s, d_a, a_stride, d_b, b_stride, d_scalars, d_out, out_stride, d_out_inf, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_g1_mul_add_batch(const uint8_t* a, size_t a_stride, const uint8_t* b, size_t b_stride, const uint8_t* scalars, uint8_t* out, uint8_t* out_inf, size_t n) {
    if (n == 0) return BLSMI_OK;
    if (!a || !b || !scalars || !out || !out_inf || !mul_add_stride_ok(a_stride) || !mul_add_stride_ok(b_stride) || n > 0xffffffffull) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    const size_t ab = mul_add_span(a_stride, n), bb = mul_add_span(b_stride, n);
    DBuf da, db, ds, dout, dinf;
    HIPCHK(da.alloc(ab)); HIPCHK(db.alloc(bb)); HIPCHK(ds.alloc((size_t)32 * n)); HIPCHK(dout.alloc((size_t)96 * n)); HIPCHK(dinf.alloc(n));
    HIPCHK(hipMemcpyAsync(da.p, a, ab, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(db.p, b, bb, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(ds.p, scalars, (size_t)32 * n, hipMemcpyHostToDevice, s));
    int rc = mul_add_dev_core(da.as<u8>(), a_stride, db.as<u8>(), b_stride, ds.as<u8>(), dout.as<u8>(), 96, dinf.as<u8>(), n, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)96 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_inf, dinf.p, n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
BLSMI_API int blsmi_g1_mul_add_batch_dev(const void* d_a, size_t a_stride, const void* d_b, size_t b_stride, const void* d_scalars, void* d_out, void* d_out_inf, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_a || !d_b || !d_scalars || !d_out || !d_out_inf || !mul_add_stride_ok(a_stride) || !mul_add_stride_ok(b_stride) || n > 0xffffffffull) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    int rc = mul_add_dev_core((const u8*)d_a, a_stride, (const u8*)d_b, b_stride, (const u8*)d_scalars, (u8*)d_out, 96, (u8*)d_out_inf, n, g_stream); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}

// m openings under the block equations of 0.18.  Item j holds when e(C_j - y_j G + z_j pi_j, H) e(pi_j, -tau H) = 1 -- tau H is negated once
// (k_g2_neg_records), no proof is.  With W_j = C_j + z_j pi_j and the weights r_j, over a block b,
//     sum_j r_j (W_j - y_j G) = sum_j r_j W_j - s_b G,        s_b = sum_j r_j y_j mod r,
// so that a block needs one scalar from the fold and one full-width ladder over -G, whatever its length; no y_j G exists on the path that
// holds.  Stages:
//   1  the plan of 0.18 over two pairs per item, (W_j, H) and (pi_j, -tau H): per block an H cell and a -tau H cell, and one further cell
//      per block appended to it (pprod_locate_append_cells) against H again: s_b (-G).  Three Miller loops per block.
//   2  the lift, its own: k_g1_mul_add_glv writes W_j = C_j + z_j pi_j into the even records of the interleaved (W_j, pi_j) buffer, read from
//      where C_j and pi_j lie; k_kzg_place_proofs copies pi_j beside it
//   3  pprod_weighted_sums, unchanged, with room for the B sums it does not make
//   4  its own: fr_wsum_dev over y with one column and the blocks as segments; B ladders of s_b over copies of -G (mul_dev_core), written
//      straight into those places -- s_b = 0 gives the infinity record and its flag, and the route leaves the cell out
//   5  pprod_locate_failing_blocks, unchanged: route, Miller loops, block products, total, final exponentiation; the failing blocks
//   6  kzg_recheck for their items only: y_j mod r (the fold again, a segment per item, weight one), y_j (-G) ladders, the two-point
//      segmented sum with the W_j already there, the two pairs dense (k_kzg_recheck_pairs), pprod_recheck_dense.  The lift runs once.
// One lease, one device, never in the request combiner.
namespace {
struct KzgIn {
    const u8* g;             // G: one affine record, 4-byte aligned
    u8* wp;                  // (W_j, pi_j) interleaved: 2 m affine records, the call's own, 16-byte aligned; the lift has filled it
    const u8* tab;           // H, -tau H: the call's own, affine
    const u8* y;             // m scalars, 4-byte aligned
    const uint64_t* r;       // host: m nonzero scalars
    size_t m, block;         // block: resolved, >= 1
};
// [k] (-G) for the n scalars k in column 1 of the fold's output d_fold (rows of two), as n affine records at d_out with their infinity bytes
// (the buffers and the index vector are the driver's: they outlive the stream's work)
struct KzgLadderBufs { std::vector<uint32_t> col; DBuf idx, scal, pts; };
int kzg_neg_g_ladders(const KzgIn& in, const void* d_fold, size_t n, u8* d_out, u8* d_out_inf, KzgLadderBufs& lb, hipStream_t s) {
    DBuf &idx = lb.idx, &scal = lb.scal, &pts = lb.pts;
    try { lb.col.resize(n); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    for (size_t k = 0; k < n; k++) lb.col[k] = (uint32_t)(2 * k + 1);
    HIPCHK(idx.alloc(sizeof(uint32_t) * n)); HIPCHK(scal.alloc((size_t)32 * n)); HIPCHK(pts.alloc((size_t)96 * n));
    HIPCHK(hipMemcpyAsync(idx.p, lb.col.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
    groth16_gather(d_fold, idx, scal.p, 32, n, s);
    launch_quiet(KERNEL_OF(k_kzg_neg_g1_copies), nblocks(n), s, in.g, pts.p, n);
    return mul_dev_core(group_kernels(1), pts.as<u8>(), scal.as<u8>(), d_out, d_out_inf, n, s);
}
// Stage 6.  items: the openings of the failing blocks, ascending.  Synchronises.
int kzg_recheck(const KzgIn& in, const PprodCall& c, const std::vector<uint32_t>& items, void* d_ok) {
    const size_t nre = items.size();
    hipStream_t s = g_stream;
    const GroupKernels& g = group_kernels(1);
    std::vector<uint64_t> ones, roff, zoff; std::vector<uint32_t> wi, zi;
    FrWsumPlan rp; SegPlan zplan, iplan;
    try {
        ones.assign(nre, 1); roff.resize(nre + 1); zoff.resize(nre + 1); wi.resize(nre); zi.resize(2 * nre);
        for (size_t t = 0; t <= nre; t++) { roff[t] = t; zoff[t] = 2 * t; }
        for (size_t t = 0; t < nre; t++) { wi[t] = 2 * items[t]; zi[2 * t] = (uint32_t)t; zi[2 * t + 1] = (uint32_t)(nre + t); }
        fr_wsum_plan(roff.data(), nre, 1, rp); segsum_plan(zoff.data(), nre, segsum_chunk_of(2 * nre), zplan); pprod_plan(zoff.data(), nre, iplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    DBuf ditems, dwi, dzi, rows, dones, rout, Z, zinf, P, Pinf, a, b, fl, okd; KzgLadderBufs lb;
    HIPCHK(ditems.alloc(sizeof(uint32_t) * nre)); HIPCHK(dwi.alloc(sizeof(uint32_t) * nre)); HIPCHK(dzi.alloc(sizeof(uint32_t) * 2 * nre));
    HIPCHK(rows.alloc((size_t)32 * nre)); HIPCHK(dones.alloc(sizeof(uint64_t) * nre)); HIPCHK(rout.alloc((size_t)64 * nre));
    HIPCHK(Z.alloc((size_t)96 * 2 * nre)); HIPCHK(zinf.alloc(2 * nre)); HIPCHK(P.alloc((size_t)96 * nre)); HIPCHK(Pinf.alloc(nre));
    HIPCHK(a.alloc((size_t)96 * 2 * nre)); HIPCHK(b.alloc((size_t)192 * 2 * nre)); HIPCHK(fl.alloc(2 * nre)); HIPCHK(okd.alloc(nre));
    HIPCHK(hipMemcpyAsync(ditems.p, items.data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dwi.p, wi.data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dzi.p, zi.data(), sizeof(uint32_t) * 2 * nre, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dones.p, ones.data(), sizeof(uint64_t) * nre, hipMemcpyHostToDevice, s));
    prof_mark(KERNEL_OF(k_gather_records16).name);                         // one segment: the gathers
    groth16_gather(in.y, ditems, rows.p, 32, nre, s);
    groth16_gather(in.wp, dwi, Z.p, 96, nre, s);                           // W_j, with the flag byte its pair got (bit 0: at infinity)
    launch_quiet(KERNEL_OF(k_gather_bytes), nblocks(nre), s, c.pflag.p, dwi.p, zinf.p, nre);
    prof_mark(nullptr);
    int rc = fr_wsum_dev(rp, rows.p, 1, dones.p, nre, rout.p, s); if (rc) return rc;   // every row: 1, y_j mod r
    rc = kzg_neg_g_ladders(in, rout.p, nre, Z.as<u8>() + (size_t)96 * nre, zinf.as<u8>() + nre, lb, s); if (rc) return rc;
    rc = segsum_dev(g, false, Z.p, zinf.as<u8>(), 2 * nre, dzi.as<u32>(), zplan, P.as<u8>(), Pinf.as<u8>(), 1, s); if (rc) return rc;
    launch(KERNEL_OF(k_kzg_recheck_pairs), tuple_blocks(Layout::row, 2 * nre), s, P.p, Pinf.p, in.wp, in.tab, ditems.p, in.m, a.p, b.p, fl.p, nre);
    prof_mark(nullptr);
    return pprod_recheck_dense(a.as<u8>(), b.as<u8>(), fl.as<u8>(), 2 * nre, iplan, ditems.as<u32>(), okd.p, d_ok);
}
// d_ok: m verdict bytes on the device.  Synchronises.
int kzg_core(const KzgIn& in, void* d_ok, bool* held, size_t* rechecked) {
    const size_t m = in.m, np = 2 * m;
    hipStream_t s = g_stream;
    *rechecked = 0;
    std::vector<uint64_t> seg_off, boff; std::vector<uint32_t> q_idx;
    blsmi_route::PprodLocatePlan pl; blsmi_route::PprodLocateFailing ff;
    FrWsumPlan fp;
    PprodCall c; PprodCellBufs b;
    size_t C0 = 0, B = 0;
    try {
        seg_off.resize(m + 1); q_idx.resize(np);
        for (size_t j = 0; j < m; j++) { seg_off[j] = 2 * j; q_idx[2 * j] = 0; q_idx[2 * j + 1] = 1; }
        seg_off[m] = np;
        if (!blsmi_route::pprod_locate_plan(seg_off.data(), m, q_idx.data(), np, 2, in.block, pl)) return BLSMI_E_ARG;   // stage 1
        C0 = pl.cells(); B = pl.blocks();
        const uint32_t further[1] = {0};                                   // H again: the cell of s_b (-G)
        blsmi_route::pprod_locate_append_cells(pl, further, 1);
        boff.resize(B + 1);
        for (size_t k = 0; k < B; k++) boff[k] = pl.item_lo(k);
        boff[B] = m;
        fr_wsum_plan(boff.data(), B, 1, fp); pprod_plan(pl.slot_off.data(), B, b.bplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t C = pl.cells(), dg = pl.entry_of.size();
    DBuf t, dent, fout; KzgLadderBufs lb;
    HIPCHK(t.alloc((size_t)192 * dg)); HIPCHK(dent.alloc(sizeof(uint32_t) * dg));
    HIPCHK(b.dsum.alloc(sizeof(uint32_t) * C)); HIPCHK(b.dent.alloc(sizeof(uint32_t) * C)); HIPCHK(b.bblob.alloc(b.bplan.blob.size()));
    HIPCHK(fout.alloc((size_t)64 * B));
    HIPCHK(hipMemcpyAsync(dent.p, pl.entry_of.data(), sizeof(uint32_t) * dg, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.dsum.p, pl.sum_of.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(b.dent.p, pl.entry_at.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.bblob.p, b.bplan.blob.data(), b.bplan.blob.size(), hipMemcpyHostToDevice, s));
    launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)48 * dg), s, in.tab, dent.p, t.p, 48, dg);   // the table in the plan's order
    const PprodRlcIn pin{in.wp, true, nullptr, t.as<u8>(), in.r, seg_off.data(), np, m};
    int rc = pprod_weighted_sums(c, pin, pprod_segments(pl, pl.cell_off, B), B, route_load(C)); if (rc) return rc;   // stage 3
    rc = fr_wsum_dev(fp, in.y, 1, c.dr.p, B, fout.p, s); if (rc) return rc;   // stage 4: every block: t_b, s_b
    rc = kzg_neg_g_ladders(in, fout.p, B, c.S.as<u8>() + (size_t)96 * C0, c.sinf.as<u8>() + C0, lb, s); if (rc) return rc;
    rc = pprod_locate_failing_blocks(c, pl, b, d_ok, held, ff);             // stage 5
    if (rc || *held) return rc;
    if (ff.items.empty()) { HIPCHK(hipStreamSynchronize(s)); return BLSMI_OK; }   // (cannot be: the total is the product of the block values)
    rc = kzg_recheck(in, c, ff.items, d_ok);                                // stage 6
    if (!rc) *rechecked = ff.items.size();
    return rc;
}
// What every form checks before any device work; m beyond 2^31 - 2 is refused (the pairs W_j, pi_j are 32-bit indices).
int kzg_check_args(bool pointers_ok, size_t m, const uint64_t* scalars) {
    if (m > 0x7ffffffeull || !pointers_ok) return BLSMI_E_ARG;
    return rlc_check_args(true, scalars, m);
}
const uint32_t KZG_TAU_H[1] = {1};                                        // srs_g2 is H, tau H
// H and -tau H, the call's table, from the key's two affine records on the device (4-byte aligned)
int kzg_table(const void* d_srs_g2_aff, u8* d_tab, hipStream_t s) {
    DBuf order; HIPCHK(order.alloc(sizeof KZG_TAU_H));
    HIPCHK(hipMemcpyAsync(order.p, KZG_TAU_H, sizeof KZG_TAU_H, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d_tab, d_srs_g2_aff, 192, hipMemcpyDeviceToDevice, s));
    launch_quiet(KERNEL_OF(k_g2_neg_records), 1, s, d_srs_g2_aff, order.p, d_tab + 192, 1);
    return BLSMI_OK;
}
// Stage 2: W_j = C_j + z_j pi_j and pi_j into the interleaved buffer.  d_c, d_p: m affine records each, 4-byte aligned.
int kzg_lift(const u8* d_c, const u8* d_p, const u8* d_z, u8* d_wp, size_t m, hipStream_t s) {
    DBuf winf; HIPCHK(winf.alloc(m));                                      // (the sums read the all-zero record; released in stream order)
    int rc = mul_add_dev_core(d_c, 96, d_p, 96, d_z, d_wp, 192, winf.as<u8>(), m, s); if (rc) return rc;
    launch_quiet(KERNEL_OF(k_kzg_place_proofs), nblocks((size_t)24 * m), s, d_p, d_wp, m);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
// The values of a blob batch (blsmi 0.21, below): y_j = p_j(z_j) is not given but evaluated into the call's own buffer, from m polynomials
// in evaluation form; everything after that is the same call.  polys / noncanon: host pointers in kzg_host, device pointers in kzg_dev_api.
struct KzgBlob { const void* polys; unsigned log2n; int order; void* noncanon; };
bool fr_eval_shape_ok(unsigned log2n, int order, size_t m);
int fr_eval_dev_core(const void* d_polys, unsigned log2n, int order, const void* d_z, void* d_y, void* d_noncanon, size_t m, hipStream_t s);
int kzg_host(const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* commitments, const uint8_t* proofs, const uint8_t* z, const uint8_t* y, size_t m,
             const uint64_t* scalars, size_t block, uint8_t* ok, int* combined, size_t* rechecked, bool jac, const KzgBlob* blob = nullptr) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = kzg_check_args(srs_g1 && srs_g2 && commitments && proofs && z && (blob ? blob->polys != nullptr : y != nullptr) && ok, m, scalars); if (rc) return rc;
    if (blob && !fr_eval_shape_ok(blob->log2n, blob->order, m)) return BLSMI_E_ARG;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    DBuf g, k2, dc, dp, dz, dy, wp, tab, dok;
    HIPCHK(g.alloc(96)); HIPCHK(k2.alloc(192 * 2)); HIPCHK(dc.alloc((size_t)96 * m)); HIPCHK(dp.alloc((size_t)96 * m)); HIPCHK(dz.alloc((size_t)32 * m)); HIPCHK(dy.alloc((size_t)32 * m));
    HIPCHK(wp.alloc((size_t)192 * m)); HIPCHK(tab.alloc(192 * 2)); HIPCHK(dok.alloc(m));
    rc = upload_points(group_kernels(1), jac, srs_g1, g.p, 1, s); if (rc) return rc;
    rc = upload_points(group_kernels(2), jac, srs_g2, k2.p, 2, s); if (rc) return rc;
    rc = upload_points(group_kernels(1), jac, commitments, dc.p, m, s); if (rc) return rc;
    rc = upload_points(group_kernels(1), jac, proofs, dp.p, m, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dz.p, z, (size_t)32 * m, hipMemcpyHostToDevice, s));
    DBuf dpolys, dnc;
    if (blob) {
        const size_t pbytes = ((size_t)32 << blob->log2n) * m;
        HIPCHK(dpolys.alloc(pbytes)); if (blob->noncanon) HIPCHK(dnc.alloc(m));
        HIPCHK(hipMemcpyAsync(dpolys.p, blob->polys, pbytes, hipMemcpyHostToDevice, s));
        rc = fr_eval_dev_core(dpolys.p, blob->log2n, blob->order, dz.p, dy.p, dnc.p, m, s); if (rc) return rc;
    } else HIPCHK(hipMemcpyAsync(dy.p, y, (size_t)32 * m, hipMemcpyHostToDevice, s));
    rc = kzg_table(k2.p, tab.as<u8>(), s); if (rc) return rc;
    rc = kzg_lift(dc.as<u8>(), dp.as<u8>(), dz.as<u8>(), wp.as<u8>(), m, s); if (rc) return rc;
    bool held = false; size_t nre = 0;
    const KzgIn in{g.as<u8>(), wp.as<u8>(), tab.as<u8>(), dy.as<u8>(), scalars, m, block ? block : blsmi_route::pprod_locate_auto_block(m)};
    rc = kzg_core(in, dok.p, &held, &nre); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ok, dok.p, m, hipMemcpyDeviceToHost, s));
    if (blob && blob->noncanon) HIPCHK(hipMemcpyAsync(blob->noncanon, dnc.p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
// the _dev forms: affine records are read where they lie, whatever their alignment (the lift reads words); in-memory records are converted
int kzg_dev_api(const void* d_srs_g1, const void* d_srs_g2, const void* d_commitments, const void* d_proofs, const void* d_z, const void* d_y, size_t m,
                const uint64_t* scalars, size_t block, void* d_ok, int* combined, size_t* rechecked, void* stream, bool jac, const KzgBlob* blob = nullptr) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = kzg_check_args(d_srs_g1 && d_srs_g2 && d_commitments && d_proofs && d_z && (blob ? blob->polys != nullptr : d_y != nullptr) && d_ok, m, scalars); if (rc) return rc;
    if (blob && !fr_eval_shape_ok(blob->log2n, blob->order, m)) return BLSMI_E_ARG;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    hipStream_t s = g_stream;
    DBuf g, k2, dc, dp, wp, tab;
    HIPCHK(wp.alloc((size_t)192 * m)); HIPCHK(tab.alloc(192 * 2));
    const u8 *pg = (const u8*)d_srs_g1, *pc = (const u8*)d_commitments, *pp = (const u8*)d_proofs; const void* pk2 = d_srs_g2;
    if (jac) {
        HIPCHK(g.alloc(96)); HIPCHK(k2.alloc(192 * 2)); HIPCHK(dc.alloc((size_t)96 * m)); HIPCHK(dp.alloc((size_t)96 * m));
        rc = jac_to_wire_dev(group_kernels(1), d_srs_g1, g.p, nullptr, 1, s); if (rc) return rc;
        rc = jac_to_wire_dev(group_kernels(2), d_srs_g2, k2.p, nullptr, 2, s); if (rc) return rc;
        rc = jac_to_wire_dev(group_kernels(1), d_commitments, dc.p, nullptr, m, s); if (rc) return rc;
        rc = jac_to_wire_dev(group_kernels(1), d_proofs, dp.p, nullptr, m, s); if (rc) return rc;
        pg = g.as<u8>(); pk2 = k2.p; pc = dc.as<u8>(); pp = dp.as<u8>();
    }
    DBuf dy;
    if (blob) {
        HIPCHK(dy.alloc((size_t)32 * m));
        rc = fr_eval_dev_core(blob->polys, blob->log2n, blob->order, d_z, dy.p, blob->noncanon, m, s); if (rc) return rc;
        d_y = dy.p;
    }
    rc = kzg_table(pk2, tab.as<u8>(), s); if (rc) return rc;
    rc = kzg_lift(pc, pp, (const u8*)d_z, wp.as<u8>(), m, s); if (rc) return rc;
    bool held = false; size_t nre = 0;
    const KzgIn in{pg, wp.as<u8>(), tab.as<u8>(), (const u8*)d_y, scalars, m, block ? block : blsmi_route::pprod_locate_auto_block(m)};
    rc = kzg_core(in, d_ok, &held, &nre); if (rc) return rc;
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_kzg_verify_batch(const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* commitments, const uint8_t* proofs, const uint8_t* z, const uint8_t* y, size_t m,
                                     const uint64_t* scalars, size_t block, uint8_t* ok, int* combined, size_t* rechecked) {
    return kzg_host(srs_g1, srs_g2, commitments, proofs, z, y, m, scalars, block, ok, combined, rechecked, false);
}
BLSMI_API int blsmi_kzg_verify_batch_jac(const uint64_t* srs_g1_jac, const uint64_t* srs_g2_jac, const uint64_t* commitments_jac, const uint64_t* proofs_jac, const uint8_t* z, const uint8_t* y, size_t m,
                                         const uint64_t* scalars, size_t block, uint8_t* ok, int* combined, size_t* rechecked) {
    return kzg_host(reinterpret_cast<const uint8_t*>(srs_g1_jac), reinterpret_cast<const uint8_t*>(srs_g2_jac), reinterpret_cast<const uint8_t*>(commitments_jac),
                    reinterpret_cast<const uint8_t*>(proofs_jac), z, y, m, scalars, block, ok, combined, rechecked, true);
}
BLSMI_API int blsmi_kzg_verify_batch_dev(const void* d_srs_g1, const void* d_srs_g2, const void* d_commitments, const void* d_proofs, const void* d_z, const void* d_y, size_t m,
                                         const uint64_t* scalars, size_t block, void* d_ok, int* combined, size_t* rechecked, void* stream) {
    return kzg_dev_api(d_srs_g1, d_srs_g2, d_commitments, d_proofs, d_z, d_y, m, scalars, block, d_ok, combined, rechecked, stream, false);
}
BLSMI_API int blsmi_kzg_verify_batch_jac_dev(const void* d_srs_g1_jac, const void* d_srs_g2_jac, const void* d_commitments_jac, const void* d_proofs_jac, const void* d_z, const void* d_y, size_t m,
                                             const uint64_t* scalars, size_t block, void* d_ok, int* combined, size_t* rechecked, void* stream) {
    return kzg_dev_api(d_srs_g1_jac, d_srs_g2_jac, d_commitments_jac, d_proofs_jac, d_z, d_y, m, scalars, block, d_ok, combined, rechecked, stream, true);
}

// ---- polynomial evaluation in Fr and KZG blob batches (blsmi 0.21; include/blsmi.h "polynomial evaluation") ------------------------------
// The scalar field proper: fr.h (Montgomery product, Fermat inversion, the evaluation domains) under the kernels of k_fr_eval.hip.
namespace {
std::mutex g_fr_dom_mu;
// The table of the domain of size 2^log2n in `order` on the leased device: N + 1 Montgomery elements, the roots in position order and N^-1
// (fr.h: domain_table).  Built on the host on first use and uploaded, one allocation per (device, log2n, order), at most 2 MiB + 32 bytes
// each; kept until blsmi_shutdown (Device::fr_dom) -- a per-device constant as the generators are: blsmi_trim leaves it, blsmi_held_bytes
// does not count it.
int fr_domain_table(unsigned log2n, int order, const u32** out) {
    std::lock_guard<std::mutex> lk(g_fr_dom_mu);
    u32*& slot = tl_ctx->dev->fr_dom[log2n][order];
    if (!slot) {
        const size_t n = ((size_t)1 << log2n) + 1;
        std::vector<blsmi_fr::Fr> t;
        try { t.resize(n); } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
        blsmi_fr::domain_table(log2n, order, t.data());
        u32* d = nullptr;
        HIPCHK(hipMalloc(&d, n * sizeof(blsmi_fr::Fr)));
        if (hipMemcpy(d, t.data(), n * sizeof(blsmi_fr::Fr), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return BLSMI_E_HIP; }
        slot = d;
    }
    *out = slot;
    return BLSMI_OK;
}
// what every evaluation refuses before any device work: a domain beyond 2^16, an order that is neither, m beyond 32 bits, m N 32 bytes
// beyond a size_t
bool fr_eval_shape_ok(unsigned log2n, int order, size_t m) {
    if (log2n > blsmi_fr::MAX_LOG2N || (order != 0 && order != 1) || m > 0xffffffffull) return false;
    return m <= (SIZE_MAX >> (log2n + 5));
}
constexpr size_t FR_EVAL_MAX_GRID = (size_t)1 << 20;                        // workgroups of an evaluation launch; each strides over the polynomials
// y_j = p_j(z_j) on s, not synchronised: the three launches, one profile segment each.  d_noncanon may be null.
int fr_eval_dev_core(const void* d_polys, unsigned log2n, int order, const void* d_z, void* d_y, void* d_noncanon, size_t m, hipStream_t s) {
    const u32* tab = nullptr;
    int rc = fr_domain_table(log2n, order, &tab); if (rc) return rc;
    DBuf D, Dinv, hit;
    HIPCHK(D.alloc((size_t)32 * m)); HIPCHK(Dinv.alloc((size_t)32 * m)); HIPCHK(hit.alloc(sizeof(uint32_t) * m));
    const size_t grid = std::min(m, FR_EVAL_MAX_GRID);
    launch_sized(KERNEL_OF(k_fr_bary_prod), grid, 256, s, d_z, tab, log2n, D.p, hit.p, m);
    launch_sized(KERNEL_OF(k_fr_inv), (m + 255) / 256, 256, s, D.p, Dinv.p, m);
    launch_sized(KERNEL_OF(k_fr_bary_sum), grid, 256, s, d_polys, d_z, tab, log2n, Dinv.p, hit.p, d_y, d_noncanon, m);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
// a lane per element, on s, not synchronised; d_b null: the inverses of a, else the products
int fr_lanes_dev_core(const void* d_a, const void* d_b, void* d_out, size_t n, hipStream_t s) {
    if (d_b) launch_sized(KERNEL_OF(k_fr_mul), (n + 255) / 256, 256, s, d_a, d_b, d_out, n);
    else launch_sized(KERNEL_OF(k_fr_inv), (n + 255) / 256, 256, s, d_a, d_out, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
int fr_lanes_host(const uint8_t* a, const uint8_t* b, bool two, uint8_t* out, size_t n) {
    if (n == 0) return BLSMI_OK;
    if (!a || (two && !b) || !out || n > 0xffffffffull) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    DBuf da, db, dout;
    HIPCHK(da.alloc((size_t)32 * n)); HIPCHK(dout.alloc((size_t)32 * n));
    HIPCHK(hipMemcpyAsync(da.p, a, (size_t)32 * n, hipMemcpyHostToDevice, s));
    if (two) { HIPCHK(db.alloc((size_t)32 * n)); HIPCHK(hipMemcpyAsync(db.p, b, (size_t)32 * n, hipMemcpyHostToDevice, s)); }
    int rc = fr_lanes_dev_core(da.p, two ? db.p : nullptr, dout.p, n, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)32 * n, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
int fr_lanes_dev_api(const void* d_a, const void* d_b, bool two, void* d_out, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_a || (two && !d_b) || !d_out || n > 0xffffffffull) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    int rc = fr_lanes_dev_core(d_a, two ? d_b : nullptr, d_out, n, g_stream); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_fr_mul_batch(const uint8_t* a, const uint8_t* b, uint8_t* out, size_t n) { return fr_lanes_host(a, b, true, out, n); }
BLSMI_API int blsmi_fr_mul_batch_dev(const void* d_a, const void* d_b, void* d_out, size_t n, void* stream) { return fr_lanes_dev_api(d_a, d_b, true, d_out, n, stream); }
BLSMI_API int blsmi_fr_inv_batch(const uint8_t* a, uint8_t* out, size_t n) { return fr_lanes_host(a, nullptr, false, out, n); }
BLSMI_API int blsmi_fr_inv_batch_dev(const void* d_a, void* d_out, size_t n, void* stream) { return fr_lanes_dev_api(d_a, nullptr, false, d_out, n, stream); }
BLSMI_API int blsmi_fr_eval_batch(const uint8_t* polys, unsigned log2n, int order, const uint8_t* z, uint8_t* y, uint8_t* noncanon, size_t m) {
    if (m == 0) return BLSMI_OK;
    if (!polys || !z || !y || !fr_eval_shape_ok(log2n, order, m)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    const size_t pbytes = ((size_t)32 << log2n) * m;
    DBuf dp, dz, dy, dnc;
    HIPCHK(dp.alloc(pbytes)); HIPCHK(dz.alloc((size_t)32 * m)); HIPCHK(dy.alloc((size_t)32 * m)); if (noncanon) HIPCHK(dnc.alloc(m));
    HIPCHK(hipMemcpyAsync(dp.p, polys, pbytes, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dz.p, z, (size_t)32 * m, hipMemcpyHostToDevice, s));
    int rc = fr_eval_dev_core(dp.p, log2n, order, dz.p, dy.p, dnc.p, m, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(y, dy.p, (size_t)32 * m, hipMemcpyDeviceToHost, s));
    if (noncanon) HIPCHK(hipMemcpyAsync(noncanon, dnc.p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
BLSMI_API int blsmi_fr_eval_batch_dev(const void* d_polys, unsigned log2n, int order, const void* d_z, void* d_y, void* d_noncanon, size_t m, void* stream) {
    if (m == 0) return BLSMI_OK;
    if (!d_polys || !d_z || !d_y || !fr_eval_shape_ok(log2n, order, m)) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_y);
    UseStream us(stream);
    int rc = fr_eval_dev_core(d_polys, log2n, order, d_z, d_y, d_noncanon, m, g_stream); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// m blobs: y_j = p_j(z_j) by the evaluation above into the call's own buffer, then blsmi_kzg_verify_batch* as it is (kzg_host / kzg_dev_api,
// kzg_core unchanged).
BLSMI_API int blsmi_kzg_verify_blob_batch(const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* polys, unsigned log2n, int order, const uint8_t* commitments,
                                          const uint8_t* proofs, const uint8_t* z, size_t m, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* noncanon,
                                          int* combined, size_t* rechecked) {
    const KzgBlob blob{polys, log2n, order, noncanon};
    return kzg_host(srs_g1, srs_g2, commitments, proofs, z, nullptr, m, scalars, block, ok, combined, rechecked, false, &blob);
}
BLSMI_API int blsmi_kzg_verify_blob_batch_jac(const uint64_t* srs_g1_jac, const uint64_t* srs_g2_jac, const uint8_t* polys, unsigned log2n, int order,
                                              const uint64_t* commitments_jac, const uint64_t* proofs_jac, const uint8_t* z, size_t m, const uint64_t* scalars, size_t block,
                                              uint8_t* ok, uint8_t* noncanon, int* combined, size_t* rechecked) {
    const KzgBlob blob{polys, log2n, order, noncanon};
    return kzg_host(reinterpret_cast<const uint8_t*>(srs_g1_jac), reinterpret_cast<const uint8_t*>(srs_g2_jac), reinterpret_cast<const uint8_t*>(commitments_jac),
                    reinterpret_cast<const uint8_t*>(proofs_jac), z, nullptr, m, scalars, block, ok, combined, rechecked, true, &blob);
}
BLSMI_API int blsmi_kzg_verify_blob_batch_dev(const void* d_srs_g1, const void* d_srs_g2, const void* d_polys, unsigned log2n, int order, const void* d_commitments,
                                              const void* d_proofs, const void* d_z, size_t m, const uint64_t* scalars, size_t block, void* d_ok, void* d_noncanon,
                                              int* combined, size_t* rechecked, void* stream) {
    const KzgBlob blob{d_polys, log2n, order, d_noncanon};
    return kzg_dev_api(d_srs_g1, d_srs_g2, d_commitments, d_proofs, d_z, nullptr, m, scalars, block, d_ok, combined, rechecked, stream, false, &blob);
}
BLSMI_API int blsmi_kzg_verify_blob_batch_jac_dev(const void* d_srs_g1_jac, const void* d_srs_g2_jac, const void* d_polys, unsigned log2n, int order,
                                                  const void* d_commitments_jac, const void* d_proofs_jac, const void* d_z, size_t m, const uint64_t* scalars, size_t block,
                                                  void* d_ok, void* d_noncanon, int* combined, size_t* rechecked, void* stream) {
    const KzgBlob blob{d_polys, log2n, order, d_noncanon};
    return kzg_dev_api(d_srs_g1_jac, d_srs_g2_jac, d_commitments_jac, d_proofs_jac, d_z, nullptr, m, scalars, block, d_ok, combined, rechecked, stream, true, &blob);
}

// ==== coset interpolation in Fr and KZG cell batches (blsmi 0.22; include/blsmi.h under the same title) =====================================
// From the n = 2^log2n values of a polynomial over the coset h <w> the n coefficients of its interpolant: k_fr_inv over the shifts, then
// k_fr_coset_interp (k_fr_ntt.hip; fr_ntt.h).  The twiddles are the order-0 domain table of 0.21, one per (device, log2n).
namespace {
// what every interpolation refuses before any device work: n beyond 2^10, an order that is neither, m beyond 32 bits, m n 32 bytes beyond a
// size_t
bool fr_interp_shape_ok(unsigned log2n, int order, size_t m) {
    if (log2n > blsmi_fr::NTT_MAX_LOG2N || (order != 0 && order != 1) || m > 0xffffffffull) return false;
    return m <= (SIZE_MAX >> (log2n + 5));
}
// items a workgroup of k_fr_coset_interp holds at once: its tile of 512 elements, a lane per item at n = 1
size_t fr_interp_group(unsigned log2n) { return log2n == 0 ? 256 : log2n > 9 ? 1 : (size_t)512 >> log2n; }
// on s, not synchronised: the two launches, one profile segment each.  d_shift_pow, d_flags may be null.
int fr_interp_dev_core(const void* d_vals, unsigned log2n, int order, const void* d_shifts, void* d_coeffs, void* d_shift_pow, void* d_flags, size_t m, hipStream_t s) {
    const u32* tab = nullptr;
    int rc = fr_domain_table(log2n, 0, &tab); if (rc) return rc;
    DBuf hinv;
    HIPCHK(hinv.alloc((size_t)32 * m));
    const size_t per = fr_interp_group(log2n), grid = std::min((m + per - 1) / per, FR_EVAL_MAX_GRID);
    launch_sized(KERNEL_OF(k_fr_inv), (m + 255) / 256, 256, s, d_shifts, hinv.p, m);
    launch_sized(KERNEL_OF(k_fr_coset_interp), grid, 256, s, d_vals, d_shifts, hinv.p, tab, log2n, order, d_coeffs, d_shift_pow, d_flags, m);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_fr_coset_interp_batch(const uint8_t* vals, unsigned log2n, int order, const uint8_t* shifts, uint8_t* coeffs, uint8_t* shift_pow, uint8_t* flags, size_t m) {
    if (m == 0) return BLSMI_OK;
    if (!vals || !shifts || !coeffs || !fr_interp_shape_ok(log2n, order, m)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    const size_t vbytes = ((size_t)32 << log2n) * m;
    DBuf dv, dh, dc, dsp, dfl;
    HIPCHK(dv.alloc(vbytes)); HIPCHK(dh.alloc((size_t)32 * m)); HIPCHK(dc.alloc(vbytes));
    if (shift_pow) HIPCHK(dsp.alloc((size_t)32 * m));
    if (flags) HIPCHK(dfl.alloc(m));
    HIPCHK(hipMemcpyAsync(dv.p, vals, vbytes, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dh.p, shifts, (size_t)32 * m, hipMemcpyHostToDevice, s));
    int rc = fr_interp_dev_core(dv.p, log2n, order, dh.p, dc.p, dsp.p, dfl.p, m, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(coeffs, dc.p, vbytes, hipMemcpyDeviceToHost, s));
    if (shift_pow) HIPCHK(hipMemcpyAsync(shift_pow, dsp.p, (size_t)32 * m, hipMemcpyDeviceToHost, s));
    if (flags) HIPCHK(hipMemcpyAsync(flags, dfl.p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
BLSMI_API int blsmi_fr_coset_interp_batch_dev(const void* d_vals, unsigned log2n, int order, const void* d_shifts, void* d_coeffs, void* d_shift_pow, void* d_flags, size_t m, void* stream) {
    if (m == 0) return BLSMI_OK;
    if (!d_vals || !d_shifts || !d_coeffs || !fr_interp_shape_ok(log2n, order, m)) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_coeffs);
    UseStream us(stream);
    int rc = fr_interp_dev_core(d_vals, log2n, order, d_shifts, d_coeffs, d_shift_pow, d_flags, m, g_stream); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}

// m cells under the block equations of 0.18.  Cell j -- the n values of a polynomial over h_j <w> -- holds when
//     e(C_j + h_j^n pi_j - sum_i c_ji [tau^i] G, H) e(pi_j, -[tau^n] H) = 1,        c_j the coefficients of the interpolant,
// which is the opening of 0.20 with z_j := h_j^n, y_j G := sum_i c_ji [tau^i] G and tau H := tau^n H.  With W_j = C_j + h_j^n pi_j and the
// weights r_j, over a block b,
//     sum_j r_j (W_j - sum_i c_ji [tau^i] G) = sum_j r_j W_j - sum_i s_bi [tau^i] G,        s_bi = sum_j r_j c_ji mod r,
// so that a block needs n scalars from the fold and n full-width ladders over the negated key records, whatever its length.  Stages:
//   1  the interpolation above into the call's own buffers (the drivers below): coeffs, shift_pow, flags
//   2  kzg_lift with z := shift_pow, kzg_table, as they are
//   3  the plan of 0.18 over two pairs per item, and one further cell per block appended to it against H, as kzg_core
//   4  pprod_weighted_sums, unchanged
//   5  its own: fr_wsum_dev over coeffs with n columns and the blocks as segments; the n key records negated once (k_kzg_neg_g1_records);
//      B n ladders of s_bi over gathered records (mul_dev_core), a segmented sum per block into the appended cells -- a block whose s_bi are
//      all 0 yields the infinity record and its flag, and the route leaves the cell out
//   6  pprod_locate_failing_blocks, unchanged
//   7  cell_recheck for the items of failing blocks only: n ladders c_ji (-[tau^i] G) per item, the segmented sum with the W_j already there
//      into dense P_j, k_kzg_recheck_pairs, pprod_recheck_dense.  The lift and the interpolation run once.
// One lease, one device, never in the request combiner.
namespace {
struct CellIn {
    const u8* key;           // [tau^0] G .. [tau^(n-1)] G: n affine records, 4-byte aligned
    u8* wp;                  // (W_j, pi_j) interleaved: 2 m affine records, the call's own, 16-byte aligned; the lift has filled it
    const u8* tab;           // H, -[tau^n] H: the call's own, affine
    const u8* coeffs;        // m * n scalars, fully reduced, the call's own
    const uint64_t* r;       // host: m nonzero scalars
    size_t n, m, block;      // block: resolved, >= 1
};
// Stage 7.  items: the cells of the failing blocks, ascending; negkey: the n negated key records.  Synchronises.
int cell_recheck(const CellIn& in, const PprodCall& c, const u8* negkey, const std::vector<uint32_t>& items, void* d_ok) {
    const size_t nre = items.size(), n = in.n, nl = nre * n;
    hipStream_t s = g_stream;
    const GroupKernels& g = group_kernels(1);
    std::vector<uint64_t> zoff, ioff; std::vector<uint32_t> wi, zi, lp;
    SegPlan zplan, iplan;
    try {
        zoff.resize(nre + 1); ioff.resize(nre + 1); wi.resize(nre); zi.resize(nre + nl); lp.resize(nl);
        for (size_t t = 0; t <= nre; t++) { zoff[t] = t * (n + 1); ioff[t] = 2 * t; }
        for (size_t t = 0; t < nre; t++) {
            wi[t] = 2 * items[t];
            zi[t * (n + 1)] = (uint32_t)t;                                  // W_j, then the item's n ladders
            for (size_t i = 0; i < n; i++) { zi[t * (n + 1) + 1 + i] = (uint32_t)(nre + t * n + i); lp[t * n + i] = (uint32_t)i; }
        }
        segsum_plan(zoff.data(), nre, segsum_chunk_of(nre + nl), zplan); pprod_plan(ioff.data(), nre, iplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    DBuf ditems, dwi, dzi, dlp, rows, lpts, Z, zinf, P, Pinf, a, b, fl, okd;
    HIPCHK(ditems.alloc(sizeof(uint32_t) * nre)); HIPCHK(dwi.alloc(sizeof(uint32_t) * nre)); HIPCHK(dzi.alloc(sizeof(uint32_t) * (nre + nl))); HIPCHK(dlp.alloc(sizeof(uint32_t) * nl));
    HIPCHK(rows.alloc((size_t)32 * nl)); HIPCHK(lpts.alloc((size_t)96 * nl));
    HIPCHK(Z.alloc((size_t)96 * (nre + nl))); HIPCHK(zinf.alloc(nre + nl)); HIPCHK(P.alloc((size_t)96 * nre)); HIPCHK(Pinf.alloc(nre));
    HIPCHK(a.alloc((size_t)96 * 2 * nre)); HIPCHK(b.alloc((size_t)192 * 2 * nre)); HIPCHK(fl.alloc(2 * nre)); HIPCHK(okd.alloc(nre));
    HIPCHK(hipMemcpyAsync(ditems.p, items.data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dwi.p, wi.data(), sizeof(uint32_t) * nre, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dzi.p, zi.data(), sizeof(uint32_t) * (nre + nl), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dlp.p, lp.data(), sizeof(uint32_t) * nl, hipMemcpyHostToDevice, s));
    prof_mark(KERNEL_OF(k_gather_records16).name);                         // one segment: the gathers
    groth16_gather(in.coeffs, ditems, rows.p, (size_t)32 * n, nre, s);     // the items' coefficient rows: n scalars each
    groth16_gather(negkey, dlp, lpts.p, 96, nl, s);
    groth16_gather(in.wp, dwi, Z.p, 96, nre, s);                           // W_j, with the flag byte its pair got (bit 0: at infinity)
    launch_quiet(KERNEL_OF(k_gather_bytes), nblocks(nre), s, c.pflag.p, dwi.p, zinf.p, nre);
    prof_mark(nullptr);
    int rc = mul_dev_core(g, lpts.as<u8>(), rows.as<u8>(), Z.as<u8>() + (size_t)96 * nre, zinf.as<u8>() + nre, nl, s); if (rc) return rc;
    rc = segsum_dev(g, false, Z.p, zinf.as<u8>(), nre + nl, dzi.as<u32>(), zplan, P.as<u8>(), Pinf.as<u8>(), 1, s); if (rc) return rc;
    launch(KERNEL_OF(k_kzg_recheck_pairs), tuple_blocks(Layout::row, 2 * nre), s, P.p, Pinf.p, in.wp, in.tab, ditems.p, in.m, a.p, b.p, fl.p, nre);
    prof_mark(nullptr);
    return pprod_recheck_dense(a.as<u8>(), b.as<u8>(), fl.as<u8>(), 2 * nre, iplan, ditems.as<u32>(), okd.p, d_ok);
}
// d_ok: m verdict bytes on the device.  Synchronises.
int cell_core(const CellIn& in, void* d_ok, bool* held, size_t* rechecked) {
    const size_t m = in.m, n = in.n, np = 2 * m, cols = n + 1;
    hipStream_t s = g_stream;
    const GroupKernels& g = group_kernels(1);
    *rechecked = 0;
    std::vector<uint64_t> seg_off, boff, goff; std::vector<uint32_t> q_idx, lpt, lsc;
    blsmi_route::PprodLocatePlan pl; blsmi_route::PprodLocateFailing ff;
    FrWsumPlan fp; SegPlan gplan;
    PprodCall c; PprodCellBufs b;
    size_t C0 = 0, B = 0, nl = 0;
    try {
        seg_off.resize(m + 1); q_idx.resize(np);
        for (size_t j = 0; j < m; j++) { seg_off[j] = 2 * j; q_idx[2 * j] = 0; q_idx[2 * j + 1] = 1; }
        seg_off[m] = np;
        if (!blsmi_route::pprod_locate_plan(seg_off.data(), m, q_idx.data(), np, 2, in.block, pl)) return BLSMI_E_ARG;   // stage 3
        C0 = pl.cells(); B = pl.blocks(); nl = B * n;
        const uint32_t further[1] = {0};                                   // H again: the cell of -sum_i s_bi [tau^i] G
        blsmi_route::pprod_locate_append_cells(pl, further, 1);
        boff.resize(B + 1); goff.resize(B + 1); lpt.resize(nl); lsc.resize(nl);
        for (size_t k = 0; k < B; k++) {
            boff[k] = pl.item_lo(k); goff[k] = k * n;
            for (size_t i = 0; i < n; i++) { lpt[k * n + i] = (uint32_t)i; lsc[k * n + i] = (uint32_t)(k * cols + 1 + i); }   // s_bi (-[tau^i] G)
        }
        boff[B] = m; goff[B] = nl;
        fr_wsum_plan(boff.data(), B, n, fp); segsum_plan(goff.data(), B, segsum_chunk_of(nl), gplan); pprod_plan(pl.slot_off.data(), B, b.bplan);
    } catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    const size_t C = pl.cells(), dg = pl.entry_of.size();
    DBuf t, dent, fout, negkey, dlp, dls, lpts, lscal, lout, linf;
    HIPCHK(t.alloc((size_t)192 * dg)); HIPCHK(dent.alloc(sizeof(uint32_t) * dg));
    HIPCHK(b.dsum.alloc(sizeof(uint32_t) * C)); HIPCHK(b.dent.alloc(sizeof(uint32_t) * C)); HIPCHK(b.bblob.alloc(b.bplan.blob.size()));
    HIPCHK(fout.alloc((size_t)32 * cols * B)); HIPCHK(negkey.alloc((size_t)96 * n)); HIPCHK(dlp.alloc(sizeof(uint32_t) * nl)); HIPCHK(dls.alloc(sizeof(uint32_t) * nl));
    HIPCHK(lpts.alloc((size_t)96 * nl)); HIPCHK(lscal.alloc((size_t)32 * nl)); HIPCHK(lout.alloc((size_t)96 * nl)); HIPCHK(linf.alloc(nl));
    HIPCHK(hipMemcpyAsync(dent.p, pl.entry_of.data(), sizeof(uint32_t) * dg, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.dsum.p, pl.sum_of.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(b.dent.p, pl.entry_at.data(), sizeof(uint32_t) * C, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(b.bblob.p, b.bplan.blob.data(), b.bplan.blob.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dlp.p, lpt.data(), sizeof(uint32_t) * nl, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dls.p, lsc.data(), sizeof(uint32_t) * nl, hipMemcpyHostToDevice, s));
    launch_quiet(KERNEL_OF(k_gather_records), nblocks((size_t)48 * dg), s, in.tab, dent.p, t.p, 48, dg);   // the table in the plan's order
    launch_quiet(KERNEL_OF(k_kzg_neg_g1_records), nblocks(n), s, in.key, negkey.p, n);
    const PprodRlcIn pin{in.wp, true, nullptr, t.as<u8>(), in.r, seg_off.data(), np, m};
    int rc = pprod_weighted_sums(c, pin, pprod_segments(pl, pl.cell_off, B), B, route_load(C)); if (rc) return rc;   // stage 4
    rc = fr_wsum_dev(fp, in.coeffs, n, c.dr.p, B, fout.p, s); if (rc) return rc;   // stage 5: every block: t_b, s_b0 .. s_b(n-1)
    groth16_gather(negkey.p, dlp, lpts.p, 96, nl, s);
    groth16_gather(fout.p, dls, lscal.p, 32, nl, s);
    rc = mul_dev_core(g, lpts.as<u8>(), lscal.as<u8>(), lout.as<u8>(), linf.as<u8>(), nl, s); if (rc) return rc;
    rc = segsum_dev(g, false, lout.p, linf.as<u8>(), nl, nullptr, gplan, c.S.as<u8>() + (size_t)96 * C0, c.sinf.as<u8>() + C0, 1, s); if (rc) return rc;
    rc = pprod_locate_failing_blocks(c, pl, b, d_ok, held, ff);             // stage 6
    if (rc || *held) return rc;
    if (ff.items.empty()) { HIPCHK(hipStreamSynchronize(s)); return BLSMI_OK; }   // (cannot be: the total is the product of the block values)
    rc = cell_recheck(in, c, negkey.as<u8>(), ff.items, d_ok);              // stage 7
    if (!rc) *rechecked = ff.items.size();
    return rc;
}
// What every form checks before any device work, in the order the header lists it.
int cell_check_args(bool pointers_ok, unsigned log2n, int order, size_t m, const uint64_t* scalars) {
    if (!pointers_ok || log2n > blsmi_fr::NTT_MAX_LOG2N || (order != 0 && order != 1) || m > 0x7ffffffeull || m > (SIZE_MAX >> (log2n + 5))) return BLSMI_E_ARG;
    return rlc_check_args(true, scalars, m);
}
int cell_host(const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* vals, unsigned log2n, int order, const uint8_t* shifts, const uint8_t* commitments,
              const uint8_t* proofs, size_t m, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* flags, int* combined, size_t* rechecked, bool jac) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = cell_check_args(srs_g1 && srs_g2 && vals && shifts && commitments && proofs && ok, log2n, order, m, scalars); if (rc) return rc;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    const size_t n = (size_t)1 << log2n, vbytes = (size_t)32 * n * m;
    DBuf g, k2, dc, dp, dv, dh, co, sp, dfl, wp, tab, dok;
    HIPCHK(g.alloc((size_t)96 * n)); HIPCHK(k2.alloc(192 * 2)); HIPCHK(dc.alloc((size_t)96 * m)); HIPCHK(dp.alloc((size_t)96 * m)); HIPCHK(dv.alloc(vbytes)); HIPCHK(dh.alloc((size_t)32 * m));
    HIPCHK(co.alloc(vbytes)); HIPCHK(sp.alloc((size_t)32 * m)); if (flags) HIPCHK(dfl.alloc(m));
    HIPCHK(wp.alloc((size_t)192 * m)); HIPCHK(tab.alloc(192 * 2)); HIPCHK(dok.alloc(m));
    rc = upload_points(group_kernels(1), jac, srs_g1, g.p, n, s); if (rc) return rc;
    rc = upload_points(group_kernels(2), jac, srs_g2, k2.p, 2, s); if (rc) return rc;
    rc = upload_points(group_kernels(1), jac, commitments, dc.p, m, s); if (rc) return rc;
    rc = upload_points(group_kernels(1), jac, proofs, dp.p, m, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(dv.p, vals, vbytes, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dh.p, shifts, (size_t)32 * m, hipMemcpyHostToDevice, s));
    rc = fr_interp_dev_core(dv.p, log2n, order, dh.p, co.p, sp.p, dfl.p, m, s); if (rc) return rc;   // stage 1
    rc = kzg_lift(dc.as<u8>(), dp.as<u8>(), sp.as<u8>(), wp.as<u8>(), m, s); if (rc) return rc;      // stage 2
    rc = kzg_table(k2.p, tab.as<u8>(), s); if (rc) return rc;
    bool held = false; size_t nre = 0;
    const CellIn in{g.as<u8>(), wp.as<u8>(), tab.as<u8>(), co.as<u8>(), scalars, n, m, block ? block : blsmi_route::pprod_locate_auto_block(m)};
    rc = cell_core(in, dok.p, &held, &nre); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ok, dok.p, m, hipMemcpyDeviceToHost, s));
    if (flags) HIPCHK(hipMemcpyAsync(flags, dfl.p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
// the _dev forms: affine records are read where they lie, whatever their alignment; in-memory records are converted
int cell_dev_api(const void* d_srs_g1, const void* d_srs_g2, const void* d_vals, unsigned log2n, int order, const void* d_shifts, const void* d_commitments,
                 const void* d_proofs, size_t m, const uint64_t* scalars, size_t block, void* d_ok, void* d_flags, int* combined, size_t* rechecked, void* stream, bool jac) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = cell_check_args(d_srs_g1 && d_srs_g2 && d_vals && d_shifts && d_commitments && d_proofs && d_ok, log2n, order, m, scalars); if (rc) return rc;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    hipStream_t s = g_stream;
    const size_t n = (size_t)1 << log2n;
    DBuf g, k2, dc, dp, co, sp, wp, tab;
    HIPCHK(co.alloc((size_t)32 * n * m)); HIPCHK(sp.alloc((size_t)32 * m)); HIPCHK(wp.alloc((size_t)192 * m)); HIPCHK(tab.alloc(192 * 2));
    const u8 *pg = (const u8*)d_srs_g1, *pc = (const u8*)d_commitments, *pp = (const u8*)d_proofs; const void* pk2 = d_srs_g2;
    if (jac) {
        HIPCHK(g.alloc((size_t)96 * n)); HIPCHK(k2.alloc(192 * 2)); HIPCHK(dc.alloc((size_t)96 * m)); HIPCHK(dp.alloc((size_t)96 * m));
        rc = jac_to_wire_dev(group_kernels(1), d_srs_g1, g.p, nullptr, n, s); if (rc) return rc;
        rc = jac_to_wire_dev(group_kernels(2), d_srs_g2, k2.p, nullptr, 2, s); if (rc) return rc;
        rc = jac_to_wire_dev(group_kernels(1), d_commitments, dc.p, nullptr, m, s); if (rc) return rc;
        rc = jac_to_wire_dev(group_kernels(1), d_proofs, dp.p, nullptr, m, s); if (rc) return rc;
        pg = g.as<u8>(); pk2 = k2.p; pc = dc.as<u8>(); pp = dp.as<u8>();
    }
    rc = fr_interp_dev_core(d_vals, log2n, order, d_shifts, co.p, sp.p, d_flags, m, s); if (rc) return rc;   // stage 1
    rc = kzg_lift(pc, pp, sp.as<u8>(), wp.as<u8>(), m, s); if (rc) return rc;                                // stage 2
    rc = kzg_table(pk2, tab.as<u8>(), s); if (rc) return rc;
    bool held = false; size_t nre = 0;
    const CellIn in{pg, wp.as<u8>(), tab.as<u8>(), co.as<u8>(), scalars, n, m, block ? block : blsmi_route::pprod_locate_auto_block(m)};
    rc = cell_core(in, d_ok, &held, &nre); if (rc) return rc;
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_kzg_verify_cell_batch(const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* vals, unsigned log2n, int order, const uint8_t* shifts,
                                          const uint8_t* commitments, const uint8_t* proofs, size_t m, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* flags,
                                          int* combined, size_t* rechecked) {
    return cell_host(srs_g1, srs_g2, vals, log2n, order, shifts, commitments, proofs, m, scalars, block, ok, flags, combined, rechecked, false);
}
BLSMI_API int blsmi_kzg_verify_cell_batch_jac(const uint64_t* srs_g1_jac, const uint64_t* srs_g2_jac, const uint8_t* vals, unsigned log2n, int order, const uint8_t* shifts,
                                              const uint64_t* commitments_jac, const uint64_t* proofs_jac, size_t m, const uint64_t* scalars, size_t block, uint8_t* ok,
                                              uint8_t* flags, int* combined, size_t* rechecked) {
    return cell_host(reinterpret_cast<const uint8_t*>(srs_g1_jac), reinterpret_cast<const uint8_t*>(srs_g2_jac), vals, log2n, order, shifts,
                     reinterpret_cast<const uint8_t*>(commitments_jac), reinterpret_cast<const uint8_t*>(proofs_jac), m, scalars, block, ok, flags, combined, rechecked, true);
}
BLSMI_API int blsmi_kzg_verify_cell_batch_dev(const void* d_srs_g1, const void* d_srs_g2, const void* d_vals, unsigned log2n, int order, const void* d_shifts,
                                              const void* d_commitments, const void* d_proofs, size_t m, const uint64_t* scalars, size_t block, void* d_ok, void* d_flags,
                                              int* combined, size_t* rechecked, void* stream) {
    return cell_dev_api(d_srs_g1, d_srs_g2, d_vals, log2n, order, d_shifts, d_commitments, d_proofs, m, scalars, block, d_ok, d_flags, combined, rechecked, stream, false);
}
BLSMI_API int blsmi_kzg_verify_cell_batch_jac_dev(const void* d_srs_g1_jac, const void* d_srs_g2_jac, const void* d_vals, unsigned log2n, int order, const void* d_shifts,
                                                  const void* d_commitments_jac, const void* d_proofs_jac, size_t m, const uint64_t* scalars, size_t block, void* d_ok,
                                                  void* d_flags, int* combined, size_t* rechecked, void* stream) {
    return cell_dev_api(d_srs_g1_jac, d_srs_g2_jac, d_vals, log2n, order, d_shifts, d_commitments_jac, d_proofs_jac, m, scalars, block, d_ok, d_flags, combined, rechecked, stream, true);
}

// ==== Fiat-Shamir challenge and KZG blob batches from wire bytes (blsmi 0.23; include/blsmi.h under the same title) ===========================
// z_j = SHA-256("FSBLOBVERIFY_V1_" || N as 16 bytes || blob_j || commitment_j) mod r by k_kzg_fs.hip (the layout and the reduction: sha256_fs.h),
// and EIP-4844's verify_blob_kzg_proof_batch composed from it: the challenge, beside it on the lease's side stream ONE k_g1_decompress launch
// over the 2 m compressed points with the subgroup test, the evaluation of 0.21 with its noncanon flags, k_kzg_wire_status, and kzg_core of
// 0.20 unchanged; k_kzg_wire_verdicts takes the verdict of every item with status != 0 back.  The decompression writes AFFINE records -- all
// zero for infinity and for a point it refuses --, which is what the lift reads: no further pass.
namespace {
enum KzgFsForm : int { FS_LANE = 0, FS_SPLIT = 1 };
constexpr int KZG_FS_DEFAULT = FS_SPLIT;                                    // the criterion and the measurement
bool kzg_fs_shape_ok(unsigned log2n, size_t m) { return fr_eval_shape_ok(log2n, 1, m); }
// on s, not synchronised; one launch, one profile segment
int kzg_fs_dev_core(const void* d_polys, unsigned log2n, const void* d_comm48, void* d_z, size_t m, int form, hipStream_t s) {
    const size_t wgs = (m + 63) / 64;
    if (form == FS_SPLIT) launch_sized(KERNEL_OF(k_kzg_fs_split), wgs, 128, s, d_polys, log2n, d_comm48, d_z, m);
    else launch_sized(KERNEL_OF(k_kzg_fs_lane), wgs, 64, s, d_polys, log2n, d_comm48, d_z, m);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
int kzg_fs_dev_api(const void* d_polys, unsigned log2n, const void* d_comm48, void* d_z, size_t m, int form, void* stream) {
    if (m == 0) return BLSMI_OK;
    if (!d_polys || !d_comm48 || !d_z || !kzg_fs_shape_ok(log2n, m) || (form != FS_LANE && form != FS_SPLIT)) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_z);
    UseStream us(stream);
    int rc = kzg_fs_dev_core(d_polys, log2n, d_comm48, d_z, m, form, g_stream); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// The call with everything on the device: d_g the key's G, d_k2 its H and tau H (affine records), the blobs and the 48-byte points where
// they lie (4-byte aligned).  d_status may be null.  Leaves the verdicts in d_ok, NOT synchronised behind the last kernel.
int kzg_wire_core(const u8* d_g, const void* d_k2, const void* d_polys, unsigned log2n, const void* d_c48, const void* d_p48, size_t m, const uint64_t* scalars, size_t block,
                  void* d_ok, void* d_status, bool overlap, bool* held, size_t* nre) {
    hipStream_t s = g_stream;
    DBuf in48, pts, pinf, perr, dz, dy, dnc, st, wp, tab;
    HIPCHK(in48.alloc((size_t)96 * m)); HIPCHK(pts.alloc((size_t)192 * m)); HIPCHK(pinf.alloc(2 * m)); HIPCHK(perr.alloc(2 * m));
    HIPCHK(dz.alloc((size_t)32 * m)); HIPCHK(dy.alloc((size_t)32 * m)); HIPCHK(dnc.alloc(m)); HIPCHK(wp.alloc((size_t)192 * m)); HIPCHK(tab.alloc(192 * 2));
    if (!d_status) { HIPCHK(st.alloc(m)); d_status = st.p; }
    // the 2 m points in one buffer: the commitments, then the proofs
    HIPCHK(hipMemcpyAsync(in48.p, d_c48, (size_t)48 * m, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(in48.as<u8>() + (size_t)48 * m, d_p48, (size_t)48 * m, hipMemcpyDeviceToDevice, s));
    const GroupKernels& g1 = group_kernels(1);
    if (overlap) {                                                         // stage 2 beside stage 1: the hash fills few waves
        HIPCHK(tl_ctx->ensure_aux());
        hipStream_t side = tl_ctx->aux[0];
        HIPCHK(hipEventRecord(tl_ctx->fork, s));
        HIPCHK(hipStreamWaitEvent(side, tl_ctx->fork, 0));
        launch_quiet(g1.decompress, nblocks(2 * m), side, in48.p, 1, pts.p, pinf.p, perr.p, 2 * m);
        HIPCHK(hipEventRecord(tl_ctx->join[0], side));
    } else launch(g1.decompress, nblocks(2 * m), s, in48.p, 1, pts.p, pinf.p, perr.p, 2 * m);
    int rc = kzg_fs_dev_core(d_polys, log2n, d_c48, dz.p, m, KZG_FS_DEFAULT, s);                             // stage 1
    if (!rc) rc = fr_eval_dev_core(d_polys, log2n, 1, dz.p, dy.p, dnc.p, m, s);                              // stage 3
    if (overlap) {                                                         // the join comes on every path: an error leaves no kernel writing the call's buffers
        if (rc) { (void)hipStreamSynchronize(tl_ctx->aux[0]); return rc; }
        HIPCHK(hipStreamWaitEvent(s, tl_ctx->join[0], 0));
    } else if (rc) return rc;
    launch_quiet(KERNEL_OF(k_kzg_wire_status), nblocks(m), s, perr.p, dnc.p, d_status, pts.p, dy.p, m);
    rc = kzg_table(d_k2, tab.as<u8>(), s); if (rc) return rc;
    rc = kzg_lift(pts.as<u8>(), pts.as<u8>() + (size_t)96 * m, dz.as<u8>(), wp.as<u8>(), m, s); if (rc) return rc;
    const KzgIn in{d_g, wp.as<u8>(), tab.as<u8>(), dy.as<u8>(), scalars, m, block ? block : blsmi_route::pprod_locate_auto_block(m)};
    rc = kzg_core(in, d_ok, held, nre); if (rc) return rc;                                                   // stage 4
    launch_quiet(KERNEL_OF(k_kzg_wire_verdicts), nblocks(m), s, d_status, d_ok, m);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
int kzg_wire_dev_api(const void* d_srs_g1, const void* d_srs_g2, const void* d_polys, unsigned log2n, const void* d_c48, const void* d_p48, size_t m, const uint64_t* scalars,
                     size_t block, void* d_ok, void* d_status, int* combined, size_t* rechecked, void* stream, bool overlap) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = kzg_check_args(d_srs_g1 && d_srs_g2 && d_polys && d_c48 && d_p48 && d_ok, m, scalars); if (rc) return rc;
    if (!kzg_fs_shape_ok(log2n, m)) return BLSMI_E_ARG;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    bool held = false; size_t nre = 0;
    rc = kzg_wire_core((const u8*)d_srs_g1, d_srs_g2, d_polys, log2n, d_c48, d_p48, m, scalars, block, d_ok, d_status, overlap, &held, &nre); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_kzg_blob_challenge_batch(const uint8_t* polys, unsigned log2n, const uint8_t* commitments48, uint8_t* z, size_t m) {
    if (m == 0) return BLSMI_OK;
    if (!polys || !commitments48 || !z || !kzg_fs_shape_ok(log2n, m)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    const size_t pbytes = ((size_t)32 << log2n) * m;
    DBuf dp, dc, dz;
    HIPCHK(dp.alloc(pbytes)); HIPCHK(dc.alloc((size_t)48 * m)); HIPCHK(dz.alloc((size_t)32 * m));
    HIPCHK(hipMemcpyAsync(dp.p, polys, pbytes, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dc.p, commitments48, (size_t)48 * m, hipMemcpyHostToDevice, s));
    int rc = kzg_fs_dev_core(dp.p, log2n, dc.p, dz.p, m, KZG_FS_DEFAULT, s); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(z, dz.p, (size_t)32 * m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
BLSMI_API int blsmi_kzg_blob_challenge_batch_dev(const void* d_polys, unsigned log2n, const void* d_commitments48, void* d_z, size_t m, void* stream) {
    return kzg_fs_dev_api(d_polys, log2n, d_commitments48, d_z, m, KZG_FS_DEFAULT, stream);
}
BLSMI_API int blsmi_debug_kzg_blob_challenge_form_dev(const void* d_polys, unsigned log2n, const void* d_commitments48, void* d_z, size_t m, int form, void* stream) {
    return kzg_fs_dev_api(d_polys, log2n, d_commitments48, d_z, m, form, stream);
}
BLSMI_API int blsmi_kzg_verify_blob_batch_wire(const uint8_t* srs_g1, const uint8_t* srs_g2, const uint8_t* polys, unsigned log2n, const uint8_t* commitments48,
                                               const uint8_t* proofs48, size_t m, const uint64_t* scalars, size_t block, uint8_t* ok, uint8_t* status, int* combined,
                                               size_t* rechecked) {
    groth16_report(combined, rechecked, false, 0);
    if (m == 0) return BLSMI_OK;
    int rc = kzg_check_args(srs_g1 && srs_g2 && polys && commitments48 && proofs48 && ok, m, scalars); if (rc) return rc;
    if (!kzg_fs_shape_ok(log2n, m)) return BLSMI_E_ARG;
    RlcHostScratch hs; uint8_t* none = nullptr;
    rc = rlc_scalars_and_ok(hs, scalars, none, false, m); if (rc) return rc;
    LOCK_AND_INIT();
    hipStream_t s = g_stream;
    const size_t pbytes = ((size_t)32 << log2n) * m;
    DBuf g, k2, dpolys, dc, dp, dok, dst;
    HIPCHK(g.alloc(96)); HIPCHK(k2.alloc(192 * 2)); HIPCHK(dpolys.alloc(pbytes)); HIPCHK(dc.alloc((size_t)48 * m)); HIPCHK(dp.alloc((size_t)48 * m));
    HIPCHK(dok.alloc(m)); HIPCHK(dst.alloc(m));
    HIPCHK(hipMemcpyAsync(g.p, srs_g1, 96, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(k2.p, srs_g2, 192 * 2, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dpolys.p, polys, pbytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dc.p, commitments48, (size_t)48 * m, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dp.p, proofs48, (size_t)48 * m, hipMemcpyHostToDevice, s));
    bool held = false; size_t nre = 0;
    rc = kzg_wire_core(g.as<u8>(), k2.p, dpolys.p, log2n, dc.p, dp.p, m, scalars, block, dok.p, dst.p, true, &held, &nre); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ok, dok.p, m, hipMemcpyDeviceToHost, s));
    if (status) HIPCHK(hipMemcpyAsync(status, dst.p, m, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    groth16_report(combined, rechecked, held, nre);
    return BLSMI_OK;
}
BLSMI_API int blsmi_kzg_verify_blob_batch_wire_dev(const void* d_srs_g1, const void* d_srs_g2, const void* d_polys, unsigned log2n, const void* d_commitments48,
                                                   const void* d_proofs48, size_t m, const uint64_t* scalars, size_t block, void* d_ok, void* d_status, int* combined,
                                                   size_t* rechecked, void* stream) {
    return kzg_wire_dev_api(d_srs_g1, d_srs_g2, d_polys, log2n, d_commitments48, d_proofs48, m, scalars, block, d_ok, d_status, combined, rechecked, stream, true);
}
BLSMI_API int blsmi_debug_kzg_verify_blob_batch_wire_dev_serial(const void* d_srs_g1, const void* d_srs_g2, const void* d_polys, unsigned log2n, const void* d_commitments48,
                                                                const void* d_proofs48, size_t m, const uint64_t* scalars, size_t block, void* d_ok, void* d_status,
                                                                int* combined, size_t* rechecked, void* stream) {
    return kzg_wire_dev_api(d_srs_g1, d_srs_g2, d_polys, log2n, d_commitments48, d_proofs48, m, scalars, block, d_ok, d_status, combined, rechecked, stream, false);
}
