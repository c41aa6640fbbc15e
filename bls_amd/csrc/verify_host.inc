// verify_host.inc -- host orchestration of the g1pubs / g2pubs verify surface (included by blsmi.hip).
// Mirrors g2pubs/bls.go:159-278 and g1pubs/bls.go:165-311; every step that touches field
// arithmetic runs in the kernels above, the host only sequences launches and checks messages for
// duplicates (a byte-string sort, g2pubs/bls.go:245-261).

namespace {

// kind 0 = g2pubs (pk in G2 192 B, sig in G1 96 B, H -> G1); 1 = g1pubs (pk in G1 96 B, sig in G2 192 B, H -> G2);
// 2 = g1pubs *WithDomain (msgs are n x 32 bytes, d_off = the 8-byte domain)
// pk_group / sig_group: the curve group (1 / 2) of the keys and of the signatures; pk() / sig(): its row for the call this thread serves
struct Kind {
    int pk_group, sig_group, pk_bytes, sig_bytes, h_bytes;
    const GroupKernels& pk() const { return group_kernels(pk_group); } const GroupKernels& sig() const { return group_kernels(sig_group); }
};
inline Kind kind_of(int kind) { return kind == 0 ? Kind{2, 1, 192, 96, 96} : Kind{1, 2, 96, 192, 192}; }

// Prepared public keys (k_prepared_pair.hip, g2pubs only): tables of blsmi_prep::WORDS i32 each on the device, and per tuple
// the index of its key's table (null: tuple t uses table t).
struct PrepKeys { const i32* tables; const u32* idx; };
// Only the lane-pair kernels read the tables in their Miller loops (route.h: prepared_tables_serve); every other layout gathers the keys'
// affine records out of the tables and runs the ordinary path (the quad kernels recompute the lines and still finish well ahead of the
// lane-pair kernels reading them: 16 384 verifies 8.3 against ~12 ms)
int prep_gather_keys(const PrepKeys& prep, DBuf& pk, size_t n, hipStream_t s) {
    HIPCHK(pk.alloc((size_t)192 * n, s));
    launch(KERNEL_OF(k_prepared_gather_keys), nblocks(48 * n), s, prep.tables, prep.idx, pk.p, n);
    prof_mark(nullptr);
    return BLSMI_OK;
}

// g1_clear == false (kind 0 only): the hash points WITHOUT their cofactor clearing (hash.cuh: swu_finish_g1), always on the throughput kernels --
// for a large g2pubs VerifyAggregate, which raises the product of its Miller values to 1 - x instead (agg_pow_wanted)
// d_special (may be null; with g1_clear == false): a device int that gets bit 1 when some message's mapped points cancel (hash.cuh: swu_finish_g1)
// r: the route of the hash (route.h: hash_route; hash_route_alone below for a hash that is the whole call)
int hash_dev(int kind, const void* d_msgs, const void* d_off_or_domain, u8* d_h, size_t n, hipStream_t s, const HashRoute& r, bool g1_clear = true, int* d_special = nullptr) {
    const unsigned g = nblocks(n), g2 = nblocks(2 * n);
    // a call in the lane-row layout (2 048 .. 8 192 tuples) hashes on the latency programs while they beat the mid-size kernels'
    // flat times (tools/midsize4.py: HashG1 two lanes + finish 1.5 ms, k_hash_g2_pair 2.9 ms; the programs take 0.27 / 0.53 ms per 1 024 messages on top of the maps)
    // HashG2 of 2 048 .. 4 096 messages (round 6): the maps and the isogeny a lane pair per message (k_hash_g2_front, an eighth of the SIMDs), then the cofactor
    // clearing -- two thirds of the hash -- sixteen lanes per message on every SIMD (k_clear_h2_row), EIGHT (k_clear_h2_oct, oct_g2.inc: the homogeneous
    // formulas' levels are four and six products wide) or four (k_clear_h2_quad, quad_g2.inc: 16 384 messages are one wave on every SIMD)
    const bool waves = r.swu == Swu::waves, rows = r.swu == Swu::rows;
    if (r.path == HashPath::lat) {
        // small batch: one lane per SWU map (the two maps of a message side by side; for the *WithDomain search two candidates
        // per round), then the curve arithmetic after the maps as a level program, one message per wave (k_lat.hip);
        // messages the program flags (good == 0) are redone by the one-lane kernel
        const size_t rec = kind == 0 ? 192 : kind == 1 ? 384 : 192;
        const size_t prog = kind == 0 ? LAT_HASHFIN1_OFFSET : kind == 1 ? LAT_HASHFIN2_OFFSET : LAT_COFAC2_OFFSET;
        DBuf pts, good; HIPCHK(pts.alloc(rec * n, s)); HIPCHK(good.alloc(n, s));
        // the smallest calls: one WAVE per SWU map, its exponentiation with one limb per lane (fp_row.cuh); then a row of sixteen lanes per map (k_hash.hip)
        if (rows && kind == 0) launch(KERNEL_OF(k_swu_g1_rows), nblocks(32 * n), s, d_msgs, d_off_or_domain, pts.p, n);
        else if (rows) launch(KERNEL_OF(k_swu_g2_rows), nblocks(32 * n), s, d_msgs, d_off_or_domain, pts.p, n);
        else if (kind == 0 && waves) launch_sized(KERNEL_OF(k_swu_g1_waves), 2 * n, 64, s, d_msgs, d_off_or_domain, pts.p, n);
        else if (kind == 1 && waves) launch_sized(KERNEL_OF(k_swu_g2_waves), 2 * n, 64, s, d_msgs, d_off_or_domain, pts.p, n);
        else if (kind == 0) launch(KERNEL_OF(k_swu_g1_two_lanes), g2, s, d_msgs, d_off_or_domain, pts.p, n);
        else if (kind == 1) launch(KERNEL_OF(k_swu_g2_two_lanes), g2, s, d_msgs, d_off_or_domain, pts.p, n);
        else if (waves) launch_sized(KERNEL_OF(k_tai_g2_waves8), n, 512, s, d_msgs, d_off_or_domain, pts.p, n);
        else launch(KERNEL_OF(k_tai_g2_lanes8), nblocks(8 * n), s, d_msgs, d_off_or_domain, pts.p, n);
        launch_lat_marked(prog, s, {.b0 = {pts.p, rec}, .ok = good.p, .out = d_h}, n);
        if (kind == 0) launch(kernel_named(k_hash_g1_redo, "k_hash_redo"), g, s, d_msgs, d_off_or_domain, good.p, d_h, n);
        else if (kind == 1) launch(kernel_named(k_hash_g2_redo, "k_hash_redo"), g, s, d_msgs, d_off_or_domain, good.p, d_h, n);
        else launch(kernel_named(k_hash_g2_domain_redo, "k_hash_redo"), g, s, d_msgs, d_off_or_domain, good.p, d_h, n);
        prof_mark(nullptr);
        HIPCHK(hipGetLastError());
        return BLSMI_OK;
    }
    // HashG1 of a mid-size batch (up to twice the quad threshold: 32 768 messages are one wave per SIMD in the two-lane kernel): the two
    // SWU maps of a message on two lanes, then the tail one message per lane -- k_hash_g1 alone leaves most SIMDs without a wave there
    if (r.path == HashPath::g1_lane || r.path == HashPath::g1_quad) {
        DBuf pts; HIPCHK(pts.alloc((size_t)192 * n, s));
        if (rows) launch(KERNEL_OF(k_swu_g1_rows), nblocks(32 * n), s, d_msgs, d_off_or_domain, pts.p, n);
        else launch(KERNEL_OF(k_swu_g1_two_lanes), g2, s, d_msgs, d_off_or_domain, pts.p, n);
        if (r.path == HashPath::g1_quad) {                                 // four lanes per message (k_hash_quad.hip, quad_g1.inc); exceptions redone a message per lane
            DBuf good; HIPCHK(good.alloc(n, s));
            launch(KERNEL_OF(k_hash_g1_finish_quad), tuple_blocks(Layout::quad, n), s, pts.p, good.p, d_h, n);
            launch(kernel_named(k_hash_g1_finish_redo, "k_hash_redo"), g, s, pts.p, good.p, d_h, n);
            prof_mark(nullptr);
            HIPCHK(hipGetLastError());
            return BLSMI_OK;
        }
        launch(KERNEL_OF(k_hash_g1_finish), g, s, pts.p, d_h, n, g1_clear ? 1 : 0, d_special);
        prof_mark(nullptr);
        HIPCHK(hipGetLastError());
        return BLSMI_OK;
    }
    // HashG2 of a large batch: a lane pair per message, two waves per SIMD (k_hash_pair.hip); BLSMI_HASH_G2_PAIR=0 keeps the one-lane kernel
    if (kind == 1 && r.path != HashPath::plain) {
        const unsigned redo_every = (unsigned)tune().hash_g2_pair_redo_every;
        DBuf good; HIPCHK(good.alloc(n, s));
        const bool g2_oct_tail = r.path == HashPath::g2_oct, g2_row_tail = r.path == HashPath::g2_row;
        if (r.path != HashPath::g2_pair) {
            DBuf jb; HIPCHK(jb.alloc(sizeof(i32) * 6 * NL_IO * n, s));
            launch(KERNEL_OF(k_hash_g2_front), g2, s, d_msgs, d_off_or_domain, good.p, jb.p, n, redo_every);
            if (g2_oct_tail) launch(KERNEL_OF(k_clear_h2_oct), (n + 7) / 8, s, jb.p, good.p, d_h, n);
            else if (g2_row_tail) launch(KERNEL_OF(k_clear_h2_row), tuple_blocks(Layout::row, n), s, jb.p, good.p, d_h, n);
            else launch(KERNEL_OF(k_clear_h2_quad), tuple_blocks(Layout::quad, n), s, jb.p, good.p, d_h, n);
            launch(kernel_named(k_hash_g2_redo, "k_hash_redo"), g, s, d_msgs, d_off_or_domain, good.p, d_h, n);
            prof_mark(nullptr);
            HIPCHK(hipGetLastError());
            return BLSMI_OK;
        }
        launch(KERNEL_OF(k_hash_g2_pair), g2, s, d_msgs, d_off_or_domain, good.p, d_h, n, redo_every);
        launch(kernel_named(k_hash_g2_redo, "k_hash_redo"), g, s, d_msgs, d_off_or_domain, good.p, d_h, n);
        prof_mark(nullptr);
        HIPCHK(hipGetLastError());
        return BLSMI_OK;
    }
    // HashG2WithDomain of a large batch in two kernels: the search and the root, one message per lane with the wave sharing its
    // messages' candidates (k_tai_g2_wave), then ScaleByCofactor with a lane pair per point at two waves per SIMD (k_cofac2_pair);
    // BLSMI_COFAC2_PAIR=0 keeps the one fused one-lane kernel
    const bool cofac_pair = tune().cofac2_pair;
    if (kind == 2 && cofac_pair) {
        DBuf pts; HIPCHK(pts.alloc((size_t)192 * n, s));
        launch(KERNEL_OF(k_tai_g2_wave), g, s, d_msgs, d_off_or_domain, pts.p, n);
        launch(KERNEL_OF(k_cofac2_pair), g2, s, pts.p, d_h, n);
        prof_mark(nullptr);
        HIPCHK(hipGetLastError());
        return BLSMI_OK;
    }
    if (kind == 0) launch(KERNEL_OF(k_hash_g1), g, s, d_msgs, d_off_or_domain, d_h, n, g1_clear ? 1 : 0, d_special);
    else if (kind == 1) launch(KERNEL_OF(k_hash_g2), g, s, d_msgs, d_off_or_domain, d_h, n);
    else launch(KERNEL_OF(k_hash_g2_domain), g, s, d_msgs, d_off_or_domain, d_h, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
// A hash that is the whole call (HashG1 / HashG2 entry points) takes the route a Verify of as many tuples gives its hash
inline HashRoute hash_route_alone(int kind, size_t n) { return hash_route(kind, n, verify_layout(n, tune(), route_load(n)), true, false, tune()); }
// one level of the Fq12 product tree: dst[t] = src[t] * src[t + half] (a missing partner counts as 1), SoA buffers of cur / half records
void launch_prod_level(const i32* src, i32* dst, size_t cur, size_t half, hipStream_t s) {
    const bool lat = half <= tune().lat_max;
    if (lat)                                                               // few products: one per wave (k_lat.hip, "mul12raw"), ~5 us instead of ~80
        launch_lat_marked(LAT_MUL12RAW_OFFSET, s, {.b2 = lat_count(half), .b3 = lat_count(cur, src), .out = dst}, half);
    else
        launch(KERNEL_OF(k_fq12_prod_level), nblocks(half), s, src, dst, cur, half);
    prof_mark(nullptr);
}
// The product tree over the cur values at src: level after level into a, b, a, ... (each with room for half the values it reads; src is never
// written, so b may be src itself); returns where the one product lies -- src when cur == 1
const i32* prod_tree(const i32* src, size_t cur, i32* a, i32* b, hipStream_t s) {
    for (i32* dst = a; cur > 1; dst = dst == a ? b : a) {
        const size_t half = (cur + 1) / 2;
        launch_prod_level(src, dst, cur, half, s);
        src = dst; cur = half;
    }
    return src;
}
// The Miller loops of an aggregate in the layout of its route (route.h: aggregate_route), which also says how many Fq12 values they leave
// in f: n, or ceil(n / 2) when two tuples share a loop.  prep: the keys' tables (only where r.tables; d_g2 is unused then).
void launch_miller1(const u8* d_g1, const u8* d_g2, i32* f, size_t n, hipStream_t s, const AggregateRoute& r, const PrepKeys* prep) {
    const size_t m = r.records;
    if (r.tables) {
        launch(KERNEL_OF(k_miller1x2_prep_pair), tuple_blocks(Layout::pair, m), s, d_g1, prep->tables, prep->idx, f, n, m);
        return;
    }
    const Layout l = r.layout;
    if (l == Layout::row)                                                  // a few thousand signers: one Miller loop per lane ROW (k_pairing_row.hip), n values as on the wave path
        launch(KERNEL_OF(k_miller1s_row), tuple_blocks(l, n), s, d_g1, 96, d_g2, 192, f, n, nullptr, 0, n);
    else if (l == Layout::wave)                                            // small aggregate: one Miller loop per wave (any Miller value serves a product that is final-exponentiated)
        launch_lat_marked(LAT_MILLER1RAW_OFFSET, s, {.b0 = {d_g1, 96}, .b1 = {d_g2, 192}, .out = f}, n);
    else if (l == Layout::quad)                                            // mid-size aggregate: two consecutive tuples per lane QUAD (k_pairing_quad.hip)
        launch(KERNEL_OF(k_miller1x2_quad), tuple_blocks(l, m), s, d_g1, d_g2, f, n, m);
    else if (l == Layout::pair)                                            // two consecutive tuples per lane pair, one 2-pair loop
        launch(KERNEL_OF(k_miller1x2_pair), tuple_blocks(l, m), s, d_g1, d_g2, f, n, m);
    else
        launch(kernels_of(l).miller1h, tuple_blocks(l, n), s, d_g1, d_g2, f, n);
}
// The signature side's Miller loop -- MillerLoop(-sig, G2One) for g2pubs, MillerLoop(-G1One, sig) for g1pubs -- needs nothing of the message,
// so it runs on a side stream WHILE the message is hashed (route.h: sig_side), its values left in f.  Small calls: program "miller1rawn", one
// wave per tuple, then "verify1s" (one Miller loop, the product, the final exponentiation): a lone g2pubs Verify 2.17 -> 2.03 ms while the side
// waves find idle SIMDs (up to 48 g2pubs / 320 g1pubs tuples, tools/side_max_probe.py).  The row layout: k_miller1s_row beside the hash, then
// k_miller1m_row (g1pubs 4 096 tuples 6.45 -> 6.10 ms, tools/midsize4.py; g2pubs with "row_side_g2pubs" and the hash's maps a lane each beside
// it: 3.55 -> 3.23 ms, profiles/r06c_variants.log).  Measured and dropped: the side kernel in pieces or with LDS reserved (r06f_side_lds.log),
// the split in the quad layout (r06_sig_side_quad_experiment.log) -- DESIGN 3e.
// after: a stream whose enqueued work produces d_sigs (null: d_sigs is complete, or host_sigs is given and copied here, on the side stream)
// sigs_jac: host_sigs are in-memory Jacobian records (converted into d_sigs on the side stream, blsmi.hip: upload_points)
// side: the call's signature side (route.h: sig_side), wave or row
// (P, Q) of the signature side's Miller loop: (sig_t, G2One) for g2pubs, (G1One, sig_t) for g1pubs, the signatures `stride` bytes apart (one
// signature: 0); the generator is the same record for every t.  launch_sig_miller: MillerLoop(-P, Q) of n such pairs into f, one wave each
// (program "miller1rawn"); the caller places its profile mark, or none on a side stream.
struct SigPair { LatBuf P, Q; };
inline SigPair sig_pair(int kind, const void* d_sigs, size_t stride) { return kind == 0 ? SigPair{{d_sigs, stride}, {g_gens.g2, 0}} : SigPair{{g_gens.g1, 0}, {d_sigs, stride}}; }
inline void launch_sig_miller(const SigPair& sp, void* f, size_t n, hipStream_t st) { launch_lat(LAT_MILLER1RAWN_OFFSET, st, {.b0 = sp.P, .b1 = sp.Q, .out = f}, n); }
int verify_sig_side_start(int kind, Side side, void* d_sigs, const uint8_t* host_sigs, i32* f, size_t n, hipStream_t after, bool sigs_jac = false) {
    const Kind k = kind_of(kind);
    HIPCHK(tl_ctx->ensure_aux());
    hipStream_t st = tl_ctx->aux[0];
    if (after) { HIPCHK(hipEventRecord(tl_ctx->fork, after)); HIPCHK(hipStreamWaitEvent(st, tl_ctx->fork, 0)); }
    if (host_sigs) { int rc = upload_points(k.sig(), sigs_jac, host_sigs, d_sigs, n, st); if (rc) return rc; }
    const SigPair sp = sig_pair(kind, d_sigs, k.sig_bytes);
    if (side == Side::row)
        launch_quiet(KERNEL_OF(k_miller1s_row), tuple_blocks(Layout::row, n), st, sp.P.p, sp.P.stride, sp.Q.p, sp.Q.stride, f, n, (kind == 0 && tune().use_gen_lines) ? (const i32*)g_gens.lines_pair : (const i32*)nullptr, 0, n);
    else
        launch_sig_miller(sp, f, n, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(tl_ctx->join[0], st));
    return BLSMI_OK;
}
// The two-pairing comparison of n tuples whose hashes h are on the device: 2-pair Miller loop, final exponentiation, == 1.
// CompareTwoPairings(sig, G2One, h, pub) (g2pubs/bls.go:161)  /  CompareTwoPairings(G1One, sig, pub, h) (g1pubs/bls.go:167, 173)
// r: the call's route (route.h: verify_route); r.side != none: the signature side's Miller values are on their way into f (verify_sig_side_start)
int verify_pair_stage(int kind, const u8* d_h, const void* d_pks, const void* d_sigs, const void* d_inf_in, void* d_ok, i32* f, size_t n, hipStream_t s, const VerifyRoute& r, const PrepKeys* prep = nullptr) {
    const unsigned g = nblocks(n), gp = tuple_blocks(Layout::pair, n);
    if (r.side != Side::none) HIPCHK(hipStreamWaitEvent(s, tl_ctx->join[0], 0));       // (also orders the side stream's copy of the signatures before the flag kernel below)
    DBuf gathered;
    if (prep && r.tables) {                       // both pairs read their lines: the generator's table and the key's
        DBuf fl; HIPCHK(fl.alloc(n, s));
        launch_quiet(KERNEL_OF(k_flag_prepared), g, s, prep->tables, prep->idx, d_sigs, 24, d_inf_in, fl.p, nullptr, n);
        launch(KERNEL_OF(k_miller2_prep_pair), gp, s, d_sigs, d_h, prep->tables, prep->idx, f, n, g_gens.lines_pair);
        launch(KERNEL_OF(k_final_exp_is_one_pair), gp, s, f, fl.p, d_ok, n);
        prof_mark(nullptr);
        HIPCHK(hipGetLastError());
        return BLSMI_OK;
    }
    if (prep) { int rc = prep_gather_keys(*prep, gathered, n, s); if (rc) return rc; d_pks = gathered.p; }
    // a key or signature at infinity (flagged by the caller, or given as the all-zero record) makes the reference panic in
    // MillerLoop (pairing.go:17-26 vs :54); here the tuple gets verdict 0
    const Kind kk = kind_of(kind);
    DBuf flags; HIPCHK(flags.alloc(n, s));
    launch_quiet(KERNEL_OF(k_flag_zero_records), g, s, d_pks, kk.pk_bytes / 4, d_sigs, kk.sig_bytes / 4, d_inf_in, flags.p, nullptr, n);
    const void* d_inf = flags.p;
    const u8* a0 = kind == 0 ? (const u8*)d_sigs : g_gens.g1; const size_t s0 = kind == 0 ? 96 : 0;
    const u8* b0 = kind == 0 ? g_gens.g2 : (const u8*)d_sigs; const size_t t0 = kind == 0 ? 0 : 192;
    const i32* pre = (kind == 0 && tune().use_gen_lines) ? g_gens.lines : nullptr;   // g2pubs: Q0 = G2 generator, prepared at start-up
    const i32* pre_pair = pre ? g_gens.lines_pair : nullptr;               // ... in the limbs of the lane-pair / lane-quad kernels
    const u8* a1 = kind == 0 ? d_h : (const u8*)d_pks;
    const u8* b1 = kind == 0 ? (const u8*)d_pks : d_h;
    if (r.side == Side::row) {                                             // lane-row layout, the signature side's Miller value already in f: the other pair's loop times it
        launch(KERNEL_OF(k_miller1m_row), tuple_blocks(Layout::row, n), s, a1, 96, b1, 192, f, n);
        launch(KERNEL_OF(k_final_exp_is_one_row), tuple_blocks(Layout::row, n), s, f, d_inf, d_ok, n);
    } else if (r.side == Side::wave) {                                     // small call, the signature side already under way: one Miller loop, the product, the final exponentiation
        launch_lat_marked(LAT_VERIFY1S_OFFSET, s, {.b0 = {a1, 96}, .b1 = {b1, 192}, .b3 = lat_count(n, f), .flags = d_inf, .ok = d_ok}, n);   // b3: the n Miller values of the side stream
    } else if (r.layout == Layout::wave) {                                 // small call: one Verify per wave (k_lat.hip)
        launch_lat_marked(LAT_VERIFY2_OFFSET, s, {.b0 = {a0, s0}, .b1 = {b0, t0}, .b2 = {a1, 96}, .b3 = {b1, 192}, .flags = d_inf, .ok = d_ok}, n);
    } else {   // row: a few thousand tuples, sixteen lanes each (k_pairing_row.hip); quad: a mid-size batch, four lanes each (k_pairing_quad.hip); pair, single
        const Layout l = r.layout;
        launch(kernels_of(l).miller2, tuple_blocks(l, n), s, a0, s0, b0, t0, a1, 96, b1, 192, f, n, l == Layout::single ? pre : pre_pair);
        launch(kernels_of(l).final_exp_is_one, tuple_blocks(l, n), s, f, d_inf, d_ok, n);
    }
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
// n independent Verify()s; everything on the device, result bytes in d_ok
// before_pair (may be null): an event the pair stage waits for -- the keys (and d_inf) are being produced on another stream while the messages are hashed
int verify_batch_dev(int kind, const void* d_msgs, const void* d_off, const void* d_pks, const void* d_sigs, const void* d_inf, void* d_ok, size_t n, hipStream_t s, const PrepKeys* prep = nullptr, hipEvent_t before_pair = nullptr) {
    if (n == 0) return BLSMI_OK;
    const Kind k = kind_of(kind);
    DBuf h, f;
    HIPCHK(h.alloc((size_t)k.h_bytes * n, s)); HIPCHK(f.alloc(sizeof(i32) * 12 * NL * n, s));
    const VerifyRoute r = verify_route(kind, n, prep != nullptr, true, tune(), route_load(n));
    if (r.side != Side::none) { int rc = verify_sig_side_start(kind, r.side, const_cast<void*>(d_sigs), nullptr, f.as<i32>(), n, s); if (rc) return rc; }   // (after s: a caller's stream may still be producing the signatures)
    int rc = hash_dev(kind, d_msgs, d_off, h.as<u8>(), n, s, r.hash);
    if (rc) return rc;
    if (before_pair) HIPCHK(hipStreamWaitEvent(s, before_pair, 0));
    rc = verify_pair_stage(kind, h.as<u8>(), d_pks, d_sigs, d_inf, d_ok, f.as<i32>(), n, s, r, prep);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
void pack_bitmap(const uint8_t* ok, uint8_t* bitmap, size_t n) {
    memset(bitmap, 0, (n + 7) / 8);
    for (size_t i = 0; i < n; i++) if (ok[i]) bitmap[i >> 3] |= (uint8_t)(1u << (i & 7));
}
// the n verdict bytes at d_ok back on the host -- in ok, or in a temporary for a caller who wants the bitmap alone --, s synchronised, the bitmap packed
int fetch_verdicts(const void* d_ok, uint8_t* ok, uint8_t* ok_bitmap, size_t n, hipStream_t s) {
    std::vector<uint8_t> tmp;
    if (!ok) { tmp.resize(n); ok = tmp.data(); }
    HIPCHK(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    if (ok_bitmap) pack_bitmap(ok, ok_bitmap, n);
    return BLSMI_OK;
}
// The messages of n > 0 tuples and their offsets on the leased context's device (kind 2: n x 32 bytes and the 8-byte domain), sized from
// the host's offsets: alloc takes the two buffers from the call's arena, copy enqueues the two uploads on s, upload does both
struct DevMsgs {
    DBuf m, off;
    size_t msg_bytes = 0, off_bytes = 0;
    DevMsgs() {}
    DevMsgs(int kind, const void* off_or_domain, size_t n)
        : msg_bytes(kind == 2 ? 32 * n : (size_t)static_cast<const uint64_t*>(off_or_domain)[n]), off_bytes(kind == 2 ? 8 : sizeof(uint64_t) * (n + 1)) {}
    int alloc() { HIPCHK(m.alloc(msg_bytes)); HIPCHK(off.alloc(off_bytes)); return BLSMI_OK; }
    int upload(const void* msgs, const void* off_or_domain, hipStream_t s) { int rc = alloc(); return rc ? rc : copy(msgs, off_or_domain, s); }
    int copy(const void* msgs, const void* off_or_domain, hipStream_t s) const {
        if (msg_bytes) HIPCHK(hipMemcpyAsync(m.p, msgs, msg_bytes, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(off.p, off_or_domain, off_bytes, hipMemcpyHostToDevice, s));
        return BLSMI_OK;
    }
};
// body of a host-buffer batch verify; the caller holds a context lease (tl_ctx)
// d_bitmap_slice (may be null): where this batch's packed verdict bits go on the lease's device (a shard of a split batch)
int verify_batch_leased(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, const uint8_t* sigs,
                        const uint8_t* inf_flags, uint8_t* ok, uint8_t* ok_bitmap, size_t n, u8* d_bitmap_slice = nullptr,
                        const i32* prep_tables = nullptr, const uint32_t* prep_idx = nullptr, int fmt = 0) {
    if (n == 0) return BLSMI_OK;
    const Kind k = kind_of(kind);
    DevMsgs dm(kind, off_or_domain, n); DBuf dp, ds, di, dok;
    { int rc = dm.alloc(); if (rc) return rc; }
    // prepared keys (resident tables): `pks` is unused, the per-tuple table indices travel in its place
    HIPCHK(dp.alloc(prep_tables ? sizeof(uint32_t) * n : (size_t)k.pk_bytes * n)); HIPCHK(ds.alloc((size_t)k.sig_bytes * n));
    HIPCHK(di.alloc(n)); HIPCHK(dok.alloc(n));
    // messages first, so that the hash-to-curve kernel runs while the (pageable, host-blocking) copies of the keys
    // and signatures are still on their way
    DBuf h, f;
    HIPCHK(h.alloc((size_t)k.h_bytes * n)); HIPCHK(f.alloc(sizeof(i32) * 12 * NL * n));
    // a small call: the signatures go first, on the side stream that runs their Miller loops beside the hash (verify_sig_side_start)
    const VerifyRoute r = verify_route(kind, n, prep_tables != nullptr, true, tune(), route_load(n));
    const bool side = r.side != Side::none;
    if (side) { int rc = verify_sig_side_start(kind, r.side, ds.p, sigs, f.as<i32>(), n, nullptr, (fmt & FMT_SIG_JAC) != 0); if (rc) return rc; }
    int rc = dm.copy(msgs, off_or_domain, g_stream);
    if (rc) return rc;
    rc = hash_dev(kind, dm.m.p, dm.off.p, h.as<u8>(), n, g_stream, r.hash);
    if (rc) return rc;
    if (prep_tables) { if (prep_idx) HIPCHK(hipMemcpyAsync(dp.p, prep_idx, sizeof(uint32_t) * n, hipMemcpyHostToDevice, g_stream)); }
    else { rc = upload_points(k.pk(), (fmt & FMT_PK_JAC) != 0, pks, dp.p, n, g_stream); if (rc) return rc; }   // (in-memory points: ToAffine on the device, after the hash)
    if (!side) { rc = upload_points(k.sig(), (fmt & FMT_SIG_JAC) != 0, sigs, ds.p, n, g_stream); if (rc) return rc; }
    if (inf_flags) HIPCHK(hipMemcpyAsync(di.p, inf_flags, n, hipMemcpyHostToDevice, g_stream));
    const PrepKeys prep{prep_tables, prep_idx ? dp.as<u32>() : nullptr};
    rc = verify_pair_stage(kind, h.as<u8>(), prep_tables ? nullptr : dp.p, ds.p, inf_flags ? di.p : nullptr, dok.p, f.as<i32>(), n, g_stream, r, prep_tables ? &prep : nullptr);
    if (rc) return rc;
    if (d_bitmap_slice) launch_quiet(KERNEL_OF(k_pack_bitmap), nblocks((n + 7) / 8), g_stream, dok.p, d_bitmap_slice, n);
    return fetch_verdicts(dok.p, ok, ok_bitmap, n, g_stream);
}

// ---- collectives of a split batch -------------------------------------------------------------------------------
// (g_coll_mu -- one split call at a time owns the per-device exchange buffers -- is declared in blsmi.hip: blsmi_trim try_locks it)
int coll_reserve_all(size_t bytes, bool zero) {
    for (int d = 0; d < g_ndev; d++) {
        HIPCHK(hipSetDevice(g_dev[d].id));
        if (!g_dev[d].coll_stream) HIPCHK(hipStreamCreateWithFlags(&g_dev[d].coll_stream, hipStreamNonBlocking));
        HIPCHK(g_dev[d].coll.reserve(bytes));
        if (zero) HIPCHK(hipMemsetAsync(g_dev[d].coll.p, 0, bytes, g_dev[d].coll_stream));
    }
    for (int d = 0; d < g_ndev; d++) { HIPCHK(hipSetDevice(g_dev[d].id)); HIPCHK(hipStreamSynchronize(g_dev[d].coll_stream)); }
    return BLSMI_OK;
}
int coll_sync_all() {
    for (int d = 0; d < g_ndev; d++) { HIPCHK(hipSetDevice(g_dev[d].id)); HIPCHK(hipStreamSynchronize(g_dev[d].coll_stream)); }
    return BLSMI_OK;
}
// the north-star's single exchange of a batch verify: every device owns the bits of its shards in a zero-initialised
// ceil(n/8)-byte map; SUM over disjoint bit ownership == OR; afterwards every device holds the whole map
// Host-staged stand-ins for the two collectives, ONLY under the BLSMI_DEVICE_ALIAS test hook (RCCL cannot put two ranks on one GPU):
// same buffers, same offsets, same result on every logical device as ncclAllReduce(uint8, SUM) / ncclAllGather.
int alias_allreduce_u8_sum(size_t nbytes) {
    std::vector<uint8_t> acc(nbytes, 0), one(nbytes);
    for (int d = 0; d < g_ndev; d++) {
        HIPCHK(hipSetDevice(g_dev[d].id));
        HIPCHK(hipMemcpyAsync(one.data(), g_dev[d].coll.p, nbytes, hipMemcpyDeviceToHost, g_dev[d].coll_stream)); HIPCHK(hipStreamSynchronize(g_dev[d].coll_stream));
        for (size_t i = 0; i < nbytes; i++) acc[i] = (uint8_t)(acc[i] + one[i]);
    }
    for (int d = 0; d < g_ndev; d++) {
        HIPCHK(hipSetDevice(g_dev[d].id));
        HIPCHK(hipMemcpyAsync(g_dev[d].coll.p, acc.data(), nbytes, hipMemcpyHostToDevice, g_dev[d].coll_stream)); HIPCHK(hipStreamSynchronize(g_dev[d].coll_stream));
    }
    return BLSMI_OK;
}
int alias_allgather(size_t send_bytes) {                                   // every device: [0, send) -> [send, send + ndev * send), rank-major
    std::vector<uint8_t> all(send_bytes * g_ndev);
    for (int d = 0; d < g_ndev; d++) {
        HIPCHK(hipSetDevice(g_dev[d].id));
        HIPCHK(hipMemcpyAsync(all.data() + send_bytes * d, g_dev[d].coll.p, send_bytes, hipMemcpyDeviceToHost, g_dev[d].coll_stream)); HIPCHK(hipStreamSynchronize(g_dev[d].coll_stream));
    }
    for (int d = 0; d < g_ndev; d++) {
        HIPCHK(hipSetDevice(g_dev[d].id));
        HIPCHK(hipMemcpyAsync((char*)g_dev[d].coll.p + send_bytes, all.data(), all.size(), hipMemcpyHostToDevice, g_dev[d].coll_stream)); HIPCHK(hipStreamSynchronize(g_dev[d].coll_stream));
    }
    return BLSMI_OK;
}
int allreduce_bitmap(size_t nbytes) {
    if (!g_have_comm) return BLSMI_OK;                                     // one device: all shards wrote into the one buffer
    if (g_alias) return alias_allreduce_u8_sum(nbytes);
    NCCLCHK(g_rccl.GroupStart());
    for (int d = 0; d < g_ndev; d++) NCCLCHK(g_rccl.AllReduce(g_dev[d].coll.p, g_dev[d].coll.p, nbytes, ncclUint8, ncclSum, g_dev[d].comm, g_dev[d].coll_stream));
    NCCLCHK(g_rccl.GroupEnd());
    return coll_sync_all();
}

int verify_batch_direct(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, const uint8_t* sigs,
                        const uint8_t* inf_flags, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int fmt = 0) {
    if (n && (!msgs || !off_or_domain || !pks || !sigs)) return BLSMI_E_ARG;
    if (n == 0) return BLSMI_OK;
    { std::lock_guard<std::mutex> lk(g_mu); int rc = ensure_init_default(); if (rc) return rc; }
    const ShardPlan plan = plan_shards(n, 64);
    if (plan.nshards == 1) {
        LOCK_AND_INIT();
        return verify_batch_leased(kind, msgs, off_or_domain, pks, sigs, inf_flags, ok, ok_bitmap, n, nullptr, nullptr, nullptr, fmt);
    }
    // split by contiguous block over the devices (g2pubs/bls.go:159 has no cross-tuple dependency); verdict bytes land in
    // the caller's array slice by slice, the bitmap goes through the all-reduce
    const Kind k = kind_of(kind);
    std::unique_lock<std::mutex> coll_lk(g_coll_mu, std::defer_lock);
    const size_t bm = (n + 7) / 8;
    if (ok_bitmap) { coll_lk.lock(); int rc = coll_reserve_all(bm, true); if (rc) return rc; }
    int rc = run_shards(plan, [&](int, size_t lo, size_t hi) -> int {
        const size_t m = hi - lo;
        std::vector<uint64_t> off_sub;
        const uint8_t* mp; const uint64_t* op;
        if (kind == 2) { mp = msgs + 32 * lo; op = off_or_domain; }
        else {
            off_sub.resize(m + 1);
            for (size_t i = 0; i <= m; i++) off_sub[i] = off_or_domain[lo + i] - off_or_domain[lo];
            mp = msgs + off_or_domain[lo]; op = off_sub.data();
        }
        u8* slice = ok_bitmap ? reinterpret_cast<u8*>(tl_ctx->dev->coll.p) + lo / 8 : nullptr;
        return verify_batch_leased(kind, mp, op, pks + rec_bytes(k.pk_bytes, fmt & FMT_PK_JAC) * lo, sigs + rec_bytes(k.sig_bytes, fmt & FMT_SIG_JAC) * lo, inf_flags ? inf_flags + lo : nullptr,
                                   ok ? ok + lo : nullptr, nullptr, m, slice, nullptr, nullptr, fmt);
    });
    if (rc) return rc;
    if (ok_bitmap) {
        rc = allreduce_bitmap(bm);
        if (rc) return rc;
        HIPCHK(hipSetDevice(g_dev[0].id));
        HIPCHK(hipMemcpyAsync(ok_bitmap, g_dev[0].coll.p, bm, hipMemcpyDeviceToHost, g_dev[0].coll_stream));
        HIPCHK(hipStreamSynchronize(g_dev[0].coll_stream));
    }
    return BLSMI_OK;
}

// ---- request combining ---------------------------------------------------------------------------------
// The Go API verifies ONE tuple per call (g2pubs/bls.go:159), and a single call costs the latency of one wave
// walking the whole path (~16 ms) however few tuples it carries -- the GPU is idle but for one lane pair.  Calls that
// arrive concurrently from many goroutines are therefore merged: the first arrival becomes the leader, waits a short
// window for company, concatenates every pending request of the same package into one batch launch and hands each
// caller its own verdicts.  While that batch runs, the next leader is already collecting the next one (it leases its
// own stream).  Throughput under concurrent single-tuple callers scales with the number of callers instead of being
// one tuple per 16 ms per stream; a lone caller pays the window (BLSMI_COMBINE_WAIT_US, default 150 us) once.
// Requests of BLSMI_COMBINE_MAX (default 1024) tuples or more bypass that queue.  BLSMI_COMBINE_MAX=0 disables it.
// Mid-size requests (BLSMI_COMBINE_MAX <= n < BLSMI_COMBINE_MID_MAX, default 8192) combine AMONG THEMSELVES, in a queue of their own (a one-tuple
// Verify never waits behind a 6-ms batch): four goroutines with 4 096 tuples each are one 16 384-tuple launch on the quad kernels -- one wave on
// every SIMD -- instead of four grids that share the chip badly (tools/midsize_concurrency.py).  A lone caller goes at once, on its own buffers.
// g1pubs *WithDomain requests (kind 2) combine with requests of the same 8-byte domain.
struct VReq {
    const uint8_t* msgs; const uint64_t* off; const uint8_t* pks; const uint8_t* sigs; const uint8_t* inf; uint8_t* ok; size_t n;
    int rc = BLSMI_OK; bool taken = false, done = false;
    uint8_t dom[8] = {0};                                                  // kind 2 (*WithDomain): requests combine when their domains agree
    std::condition_variable cv;                                            // signalled when done, or when promoted to lead
};
struct Combiner {
    std::mutex mu; std::condition_variable leader_cv;                    // the forming leader waits here for arrivals
    std::vector<VReq*> pending; bool forming = false;
    int inflight = 0; std::condition_variable slot_cv;                   // combined batches running; the next leader waits for a slot
    size_t last_requests = 0;                                            // requests in the batch formed last
} g_comb[12];                            // [kind] affine wire records, [3 + kind] in-memory Jacobian records (requests of one format combine); [6 + ...] the mid-size class
constexpr size_t g_combine_cap = 16384;
#define g_combine_max (g_env.combine_max)
#define g_combine_wait_us (g_env.combine_wait_us)
#define g_combine_inflight_max (g_env.combine_inflight_max)      // BLSMI_COMBINE_INFLIGHT: a small call costs ~3 ms whatever it carries, so few, fuller batches win
#define g_combine_debug (g_env.combine_debug)
struct Staging { std::vector<uint8_t> msgs, pks, sigs, inf, ok; std::vector<uint64_t> off; };
std::mutex g_staging_mu;
std::vector<std::unique_ptr<Staging>> g_staging_free;
constexpr size_t STAGING_KEEP = 4;
// run the requests in `batch` as one launch (on the context the leader leased) and distribute the verdicts
void combine_run(int kind, std::vector<VReq*>& batch, int fmt) {
    Kind k = kind_of(kind);
    k.pk_bytes = (int)rec_bytes(k.pk_bytes, fmt & FMT_PK_JAC); k.sig_bytes = (int)rec_bytes(k.sig_bytes, fmt & FMT_SIG_JAC);   // bytes per record as they arrive
    size_t n = 0, mbytes = 0; bool any_inf = false;
    if (batch.size() == 1) {                                               // nobody joined: the caller's own buffers, no copies
        VReq* r = batch[0];
        r->rc = verify_batch_leased(kind, r->msgs, kind == 2 ? reinterpret_cast<const uint64_t*>(r->dom) : r->off, r->pks, r->sigs, r->inf, r->ok, nullptr, r->n, nullptr, nullptr, nullptr, fmt);
        return;
    }
    for (VReq* r : batch) { n += r->n; mbytes += kind == 2 ? 32 * r->n : (size_t)r->off[r->n]; any_inf |= r->inf != nullptr; }
    // staging of the merged batch: kept between batches (a fresh 4-MB vector per mid-size batch is a millisecond of page faults) in a small shared
    // pool rather than per thread -- under cgo the leader can be any OS thread, and per-thread staging grew with the number of threads that ever led
    // a batch (ADVICE r05).  At most STAGING_KEEP sets stay allocated (one per batch in flight: BLSMI_COMBINE_INFLIGHT x the classes that merge at once).
    struct StagingLease {
        std::unique_ptr<Staging> s;
        StagingLease() { std::lock_guard<std::mutex> lk(g_staging_mu); if (!g_staging_free.empty()) { s = std::move(g_staging_free.back()); g_staging_free.pop_back(); } else s.reset(new Staging); }
        ~StagingLease() { std::lock_guard<std::mutex> lk(g_staging_mu); if (g_staging_free.size() < STAGING_KEEP) g_staging_free.push_back(std::move(s)); }
    } lease;
    std::vector<uint8_t>&msgs = lease.s->msgs, &pks = lease.s->pks, &sigs = lease.s->sigs, &inf = lease.s->inf, &ok = lease.s->ok;
    std::vector<uint64_t>& off = lease.s->off;
    msgs.resize(mbytes ? mbytes : 1); pks.resize((size_t)k.pk_bytes * n); sigs.resize((size_t)k.sig_bytes * n); inf.assign(any_inf ? n : 0, 0); ok.resize(n); off.resize(n + 1);
    size_t t = 0, mb = 0;
    off[0] = 0;
    for (VReq* r : batch) {
        const size_t rb = kind == 2 ? 32 * r->n : (size_t)r->off[r->n];
        if (rb) memcpy(msgs.data() + mb, r->msgs, rb);
        if (kind != 2) for (size_t i = 0; i < r->n; i++) off[t + i + 1] = mb + r->off[i + 1];
        memcpy(pks.data() + (size_t)k.pk_bytes * t, r->pks, (size_t)k.pk_bytes * r->n);
        memcpy(sigs.data() + (size_t)k.sig_bytes * t, r->sigs, (size_t)k.sig_bytes * r->n);
        if (r->inf) memcpy(inf.data() + t, r->inf, r->n);
        t += r->n; mb += rb;
    }
    const uint64_t* off_or_dom = kind == 2 ? reinterpret_cast<const uint64_t*>(batch[0]->dom) : off.data();    // 32-byte messages + the shared domain
    const int rc = verify_batch_leased(kind, msgs.data(), off_or_dom, pks.data(), sigs.data(), any_inf ? inf.data() : nullptr, ok.data(), nullptr, n, nullptr, nullptr, nullptr, fmt);
    t = 0;
    for (VReq* r : batch) { if (rc == BLSMI_OK) memcpy(r->ok, ok.data() + t, r->n); r->rc = rc; t += r->n; }
}
int verify_batch_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, const uint8_t* sigs,
                      const uint8_t* inf_flags, uint8_t* ok, uint8_t* ok_bitmap, size_t n, int fmt = 0) {
    // the BLSMI_COMBINE_* settings are read below: the environment must have been loaded (ADVICE r05: the first call of a process read the defaults, unsynchronised)
    { std::lock_guard<std::mutex> lk(g_mu); int rc = ensure_init_default(); if (rc) return rc; }
    const bool mid = n >= g_combine_max;                                   // the mid-size class (only where small calls combine at all)
    if (n == 0 || (mid && (g_combine_max == 0 || n >= tuning_now().combine_mid_max)) || !msgs || !off_or_domain || !pks || !sigs || (kind != 2 && off_or_domain[0] != 0) || (fmt != 0 && fmt != FMT_JAC))
        return verify_batch_direct(kind, msgs, off_or_domain, pks, sigs, inf_flags, ok, ok_bitmap, n, fmt);
    // a batch this full does not wait for more company.  With several devices a merged batch stays below the split threshold: it runs on ONE lease
    // (one device), and a direct call of BLSMI_SHARD_MIN tuples would have been cut over all of them (ADVICE r05)
    const size_t enough = mid ? ((g_ndev > 1 && g_shard_min > 1) ? std::min(g_combine_cap, g_shard_min - 1) : g_combine_cap) : g_combine_max;
    // A mid-size call merges only where it would otherwise WAIT: with a call context free, its own launch beside the others' is the better use of
    // the chip (four callers x 4 096 tuples on four contexts: 11.5 ms a call against 14.7 merged -- a merged batch serialises what four streams overlap);
    // with every context taken -- more callers than BLSMI_STREAMS -- the waiters become one launch instead of a queue (eight callers: 1.41 -> 1.95 M/s).
    if (mid && context_free_now()) return verify_batch_direct(kind, msgs, off_or_domain, pks, sigs, inf_flags, ok, ok_bitmap, n, fmt);
    std::vector<uint8_t> tmp;
    VReq me;
    if (kind == 2) memcpy(me.dom, off_or_domain, 8);
    me.msgs = msgs; me.off = off_or_domain; me.pks = pks; me.sigs = sigs; me.inf = inf_flags; me.ok = ok; me.n = n;
    if (!me.ok) { tmp.resize(n); me.ok = tmp.data(); }
    Combiner& c = g_comb[kind + (fmt ? 3 : 0) + (mid ? 6 : 0)];
    std::unique_lock<std::mutex> lk(c.mu);
    c.pending.push_back(&me);
    if (c.forming) c.leader_cv.notify_one();                             // the forming leader counts arrivals
    while (!me.done) {
        if (!c.forming && !me.taken) {                                   // lead the next batch
            c.forming = true;
            // At most g_combine_inflight_max combined batches run at a time: while this leader waits for a slot, arrivals
            // join its batch (one latency-path launch serves 1 or 1 000 tuples in the same ~3 ms).
            while (c.inflight >= g_combine_inflight_max) c.slot_cv.wait(lk);
            c.inflight++;
            // Lease the stream/scratch context BEFORE closing the batch: when every context is busy this blocks, and
            // everything that arrives meanwhile joins this batch instead of queueing as batches of its own.
            lk.unlock();
            CtxLease lease;
            lk.lock();
            if (lease.rc) {                                              // no device: fail this request, let others retry
                c.forming = false;
                c.inflight--; c.slot_cv.notify_one();
                for (auto it = c.pending.begin(); it != c.pending.end(); ++it) if (*it == &me) { c.pending.erase(it); break; }
                if (!c.pending.empty()) c.pending.front()->cv.notify_one();
                return lease.rc;
            }
            // The window for company is only worth its 150 us when there has been company: a lone caller -- nobody else
            // pending now, and the previous batch carried one request -- goes at once.
            const bool company = c.pending.size() > 1 || c.last_requests > 1;
            const auto deadline = std::chrono::steady_clock::now() + std::chrono::microseconds(company ? g_combine_wait_us : 0);
            size_t have = 0;
            for (;;) {
                have = 0;
                for (VReq* r : c.pending) have += r->n;
                if (have >= enough || !company) break;
                if (c.leader_cv.wait_until(lk, deadline) == std::cv_status::timeout) break;
            }
            std::vector<VReq*> batch, rest;
            size_t total = me.n;
            batch.push_back(&me); me.taken = true;
            for (VReq* r : c.pending) {
                if (r == &me) continue;
                if (kind == 2 && memcmp(r->dom, me.dom, 8) != 0) { rest.push_back(r); continue; }   // another domain: another batch
                if (total + r->n <= g_combine_cap) { batch.push_back(r); r->taken = true; total += r->n; } else rest.push_back(r);
            }
            c.pending.swap(rest);
            c.last_requests = batch.size();
            c.forming = false;
            if (!c.pending.empty()) c.pending.front()->cv.notify_one();  // someone left behind leads the next batch
            lk.unlock();
            const auto tr0 = std::chrono::steady_clock::now();
            combine_run(kind, batch, fmt);
            if (g_combine_debug) fprintf(stderr, "blsmi combine: kind %d batch of %zu requests / %zu tuples, ran %.2f ms\n", kind, batch.size(), total,
                                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tr0).count());
            lk.lock();
            c.inflight--; c.slot_cv.notify_one();
            for (VReq* r : batch) { r->done = true; if (r != &me) r->cv.notify_one(); }   // one wake-up per caller, no herd
        } else {
            me.cv.wait(lk);
        }
    }
    lk.unlock();
    if (me.rc == BLSMI_OK && ok_bitmap) pack_bitmap(me.ok, ok_bitmap, n);
    return me.rc;
}

// duplicate-message rejection of VerifyAggregate (g2pubs/bls.go:245-261).  lastMsg starts as nil and
// bytes.Equal(m, nil) holds for an empty m, so an empty message is rejected as well.
// The reference sorts the messages and compares neighbours; the verdict "some message occurs twice, or one is empty" is the
// same from an open-addressing table over 64-bit hashes with exact comparison on a hit: O(n) instead of n log n memcmp's (a
// million 32-byte messages: ~35 ms instead of ~180 ms).  Messages are attacker-supplied, so the hash is keyed per process
// and a probe sequence longer than 64 abandons the table for the reference's sort (n log n in the worst case).
bool has_duplicates_sorted(const uint8_t* msgs, const uint64_t* off, size_t n) {
    std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
    auto less = [&](uint32_t a, uint32_t b) {
        const size_t la = (size_t)(off[a + 1] - off[a]), lb = (size_t)(off[b + 1] - off[b]);
        const int c = memcmp(msgs + off[a], msgs + off[b], la < lb ? la : lb);
        return c ? c < 0 : la < lb;
    };
    std::sort(idx.begin(), idx.end(), less);
    if (n && off[idx[0] + 1] == off[idx[0]]) return true;                 // the first comparison is against nil: an empty message sorts first
    for (size_t i = 1; i < n; i++) if (!less(idx[i - 1], idx[i])) return true;
    return false;
}
// Process-wide key of the message fingerprints (host table below, device sort in k_util.hip): messages are
// attacker-supplied, the key is not.  std::random_device may throw on an exotic platform: fall back to the clock and ASLR.
const uint64_t* dup_key() {
    static const struct K { uint64_t k[2]; K() {
        uint64_t a, b;
        try { std::random_device rd; a = ((uint64_t)rd() << 32) ^ rd(); b = ((uint64_t)rd() << 32) ^ rd(); }
        catch (...) { a = (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count(); b = (uint64_t)(uintptr_t)&a * 0x9e3779b97f4a7c15ull ^ (a << 17); }
        k[0] = a ^ 0x9e3779b97f4a7c15ull; k[1] = b | 1;
    } } key;
    return key.k;
}
// force_sort: the "dup_force_sort" test hook -- the fallback path on every call
bool has_duplicates(const uint8_t* msgs, const uint64_t* off, size_t n, bool force_sort) {
    if (n == 0) return false;
    if (n >= 0xffffffffull) return true;                                   // not representable: treat as failure
    for (size_t i = 0; i < n; i++) if (off[i + 1] == off[i]) return true; // bytes.Equal(m, nil) holds for an empty m
    if (force_sort) return has_duplicates_sorted(msgs, off, n);
    const uint64_t* key = dup_key();
    size_t cap = 16;
    while (cap < 2 * n) cap <<= 1;
    std::vector<uint32_t> table(cap, 0);                                   // 0 = empty, else message index + 1
    for (size_t i = 0; i < n; i++) {
        const uint8_t* m = msgs + off[i];
        const size_t len = (size_t)(off[i + 1] - off[i]);
        uint64_t h = key[0] ^ (len * key[1]);
        size_t k = 0;
        for (; k + 8 <= len; k += 8) { uint64_t w; memcpy(&w, m + k, 8); h ^= w; h *= key[1]; h ^= h >> 32; h *= 0xff51afd7ed558ccdull; h ^= h >> 29; }
        uint64_t tail = 0;
        if (k < len) { memcpy(&tail, m + k, len - k); h ^= tail; h *= key[1]; h ^= h >> 32; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 29; }
        h *= 0x9e3779b97f4a7c15ull; h ^= h >> 31;
        size_t slot = (size_t)h & (cap - 1);
        for (int probes = 0;; probes++) {
            if (probes > 64) return has_duplicates_sorted(msgs, off, n);
            const uint32_t e = table[slot];
            if (e == 0) { table[slot] = (uint32_t)(i + 1); break; }
            const size_t j = e - 1;
            if ((size_t)(off[j + 1] - off[j]) == len && memcmp(msgs + off[j], m, len) == 0) return true;
            slot = (slot + 1) & (cap - 1);
        }
    }
    return false;
}
// the same verdict; an allocation failure inside (a million-entry table) is reported instead of unwinding through the C ABI
int has_duplicates_rc(const uint8_t* msgs, const uint64_t* off, size_t n, bool* dup, bool force_sort) {
    try { *dup = has_duplicates(msgs, off, n, force_sort); return BLSMI_OK; }
    catch (const std::bad_alloc&) { return BLSMI_E_NOMEM; }
    catch (...) { return BLSMI_E_ARG; }
}
bool all_zero(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) if (p[i]) return false; return true; }

// One shard of VerifyAggregate, everything resident on the device of the leased context: prod_i MillerLoop(H(m_i), pk_i)
// over n > 0 tuples (no final exponentiation), left as 180 words (an SoA buffer of one record) at d_out.  *bad (host
// memory that must stay valid until the caller synchronises s) = 1 when some key is the point at infinity (flagged
// through the all-zero record), where the reference panics in MillerLoop.  Enqueues on s and does NOT synchronise.
// after_hash (may be empty) runs once the hash-to-curve kernel has been enqueued: the host-buffer caller issues its
// (pageable, host-blocking) copy of the keys there, so that it overlaps the hash.
// g1_clear == false: see agg_pow_wanted -- d_out is then the product over the UNCLEARED hash points, to be raised to 1 - x by the caller.
int aggregate_shard_dev(int kind, const void* d_msgs, const void* d_off_or_domain, const u8* d_pks, size_t n, i32* d_out, int* bad, hipStream_t s,
                        const std::function<int()>& after_hash = {}, const PrepKeys* prep = nullptr, bool g1_clear = true) {
    const Kind k = kind_of(kind);
    DBuf gathered;
    const AggregateRoute r = aggregate_route(kind, n, prep != nullptr, g1_clear, tune(), route_load(n));   // the buffers are sized by the route the loops run by
    if (prep && !r.tables) { int rc = prep_gather_keys(*prep, gathered, n, s); if (rc) return rc; d_pks = gathered.as<u8>(); prep = nullptr; }
    const size_t words = (size_t)12 * NL;
    DBuf h, fr0, fr1, flags, any;
    const size_t nrec = r.records;
    HIPCHK(h.alloc((size_t)k.h_bytes * n, s));
    HIPCHK(fr0.alloc(sizeof(i32) * words * nrec, s)); HIPCHK(fr1.alloc(sizeof(i32) * words * ((nrec + 1) / 2), s)); HIPCHK(flags.alloc(n, s)); HIPCHK(any.alloc(sizeof(int), s));
    HIPCHK(hipMemsetAsync(any.p, 0, sizeof(int), s));
    int rc = hash_dev(kind, d_msgs, d_off_or_domain, h.as<u8>(), n, s, r.hash, g1_clear, g1_clear ? nullptr : any.as<int>());   // *bad bit 1: a hash point the uncleared path does not cover
    if (rc) return rc;
    if (after_hash) { rc = after_hash(); if (rc) return rc; }
    if (prep) launch_quiet(KERNEL_OF(k_flag_prepared), nblocks(n), s, prep->tables, prep->idx, nullptr, 0, nullptr, flags.p, any.p, n);
    else launch_quiet(KERNEL_OF(k_flag_zero_records), nblocks(n), s, d_pks, k.pk_bytes / 4, nullptr, 0, nullptr, flags.p, any.p, n);
    // Pairing(h_i, pk_i) (g2pubs) / Pairing(pk_i, h_i) (g1pubs): Miller loops only, then the product tree
    launch_miller1(kind == 0 ? h.as<u8>() : d_pks, kind == 0 ? d_pks : h.as<u8>(), fr0.as<i32>(), n, s, r, prep);
    const i32* src = prod_tree(fr0.as<i32>(), nrec, fr1.as<i32>(), fr0.as<i32>(), s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(d_out, src, sizeof(i32) * words, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(bad, any.p, sizeof(int), hipMemcpyDeviceToHost, s));
    return BLSMI_OK;                                                      // temporaries are released in stream order
}
// Host-buffer form of one shard on the leased context: copies in, runs the shard, synchronises.
int aggregate_shard(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, size_t n, i32* d_out, int* bad, bool g1_clear = true, int fmt = 0) {
    const Kind k = kind_of(kind);
    DevMsgs dm(kind, off_or_domain, n); DBuf dp;
    HIPCHK(dp.alloc((size_t)k.pk_bytes * n));
    { int rc = dm.upload(msgs, off_or_domain, g_stream); if (rc) return rc; }
    hipStream_t s = g_stream;
    int rc = aggregate_shard_dev(kind, dm.m.p, dm.off.p, dp.as<u8>(), n, d_out, bad, s, [&]() -> int {
        return upload_points(k.pk(), (fmt & FMT_PK_JAC) != 0, pks, dp.p, n, s);   // the hash runs while the keys are on their way (in-memory points: + ToAffine on the device)
    }, nullptr, g1_clear);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
// Cofactor clearing moved through the pairing (g2pubs aggregates of AGG_POW_MIN messages and more).  HashG1(m) = [1 - x] S with S the image
// of the two SWU maps on E(Fq) (hash.go:306-321).  The reduced pairing is bilinear in its E(Fq) argument modulo r E(Fq), so
// FE(ML(S, Q))^(1-x) = FE(ML([1-x] S, Q)) also for S outside the subgroup (tests/test_lat_program.py checks it on the oracle), and
//     prod_i e(H_i, pk_i) = FE( (prod_i ML(S_i, pk_i))^(1-x) ):
// the n cofactor multiplications (63 doublings + 6 additions each: 30 % of a HashG1, 8.4 ms per 2^20 messages) become ONE 64-bit
// exponentiation of the Miller product (program "powc12raw", 0.3 ms).  The verdict is the reference's; BLSMI_AGG_COFACTOR_POW=0 at start-up, or
// blsmi_set_option("agg_cofactor_pow", 0), keeps the cleared hash points.
constexpr size_t AGG_POW_MIN = 65536;
inline bool agg_pow_wanted(int kind, size_t n, const Tuning& t) { return kind == 0 && n >= AGG_POW_MIN && t.lat_max != 0 && t.agg_cofactor_pow; }
// d_prod (180 words, device representation) -> d_out = d_prod^(1 - x), on g_stream
int aggregate_pow_c(const i32* d_prod, i32* d_out) {
    launch_lat_marked(LAT_POWC12RAW_OFFSET, g_stream, {.b3 = {d_prod, 0}, .out = d_out}, 1);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
// The tuple side of an aggregate with its uncleared-hash route decided in ONE place.  run(g1_clear, &bad) enqueues the shard(s), synchronises
// and leaves the bits of aggregate_shard_dev in bad.  powc (agg_pow_wanted): the shards pair the hash points before their cofactor clearing;
// where they met a message that route does not cover (bit 1; hash.cuh: swu_finish_g1) and no key at infinity has settled the verdict anyway,
// they run once more over the cleared points and powc comes back false.  powc still true: the product wants aggregate_pow_c.
template <class Run>
int run_tuple_side(bool& powc, int* bad, const Run& run) {
    *bad = 0;
    int rc = run(!powc, bad);
    if (rc == BLSMI_OK && (*bad & 3) == 2) { powc = false; *bad = 0; rc = run(true, bad); }
    return rc;
}
// ... for a product that lies on the leased context: prod ends as the value the tail takes, raised to 1 - x where the route asks for it
// (nothing more is enqueued once *bad & 1 says that the verdict is 0)
template <class Run>
int tuple_side_product(bool powc, DBuf& prod, int* bad, const Run& run) {
    int rc = run_tuple_side(powc, bad, run);
    if (rc || (*bad & 1) || !powc) return rc;
    DBuf pc; HIPCHK(pc.alloc(sizeof(i32) * 12 * NL));
    rc = aggregate_pow_c(prod.as<i32>(), pc.as<i32>());
    prod = pc;
    return rc;
}
// one wave of a tail program ("aggtail", "aggtail2") on g_stream and its verdict byte fetched into *ok; synchronises.  a: all operands but ok
int tail_verdict(size_t prog, LatArgs a, int* ok) {
    DBuf dokb; HIPCHK(dokb.alloc(1));
    a.ok = dokb.p;
    launch_lat_marked(prog, g_stream, a, 1);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    uint8_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, dokb.p, 1, hipMemcpyDeviceToHost, g_stream)); HIPCHK(hipStreamSynchronize(g_stream));
    *ok = flag;
    return BLSMI_OK;
}
// The end of every VerifyAggregate, on the leased context: e(sig-side) == FE(prod) <=> FE(MillerLoop(-P, Q) * prod) == 1 with
// (P, Q) = (sig, G2One) / (G1One, sig).  ONE wave runs that Miller loop, the product and the single final exponentiation as a
// level program (k_lat.hip, program "aggtail") -- ~2 ms instead of a one-lane Miller loop plus two one-lane final
// exponentiations (~30 ms).  d_prod: the product of the tuple-side Miller loops (180 words on this device).
int aggregate_tail(int kind, const i32* d_prod, const uint8_t* sig, int* ok, int fmt = 0) {
    const Kind k = kind_of(kind);
    DBuf dsig; HIPCHK(dsig.alloc(k.sig_bytes));
    { int rc = upload_points(k.sig(), (fmt & FMT_SIG_JAC) != 0, sig, dsig.p, 1, g_stream); if (rc) return rc; }
    const SigPair sp = sig_pair(kind, dsig.p, 0);
    return tail_verdict(LAT_AGGTAIL_OFFSET, {.b0 = sp.P, .b1 = sp.Q, .b3 = {d_prod, 0}}, ok);
}
// The same tail in two pieces for calls that run on ONE context: the signature side's Miller loop does not depend on the tuple side, so it
// starts on a side stream BEFORE the messages are hashed (sig_side_start: program "miller1rawn", one wave, ~0.7 ms, hidden behind the
// hash and the n Miller loops), and what is left after the product tree is one product and the final exponentiation (program "aggtail2",
// ~0.85 ms instead of 1.35): 0.5 ms off every VerifyAggregate, 14 % of a 128-signer call (g1pubs/verify_benchmark_test.go:58-85).
struct SigSide { DBuf sig, ml; };
int sig_side_start(int kind, const uint8_t* sig, SigSide& ss, int fmt = 0) {
    const Kind k = kind_of(kind);
    HIPCHK(tl_ctx->ensure_aux());
    hipStream_t st = tl_ctx->aux[0];
    HIPCHK(ss.sig.alloc(k.sig_bytes)); HIPCHK(ss.ml.alloc(sizeof(i32) * 12 * NL));
    { int rc = upload_points(k.sig(), (fmt & FMT_SIG_JAC) != 0, sig, ss.sig.p, 1, st); if (rc) return rc; }
    launch_sig_miller(sig_pair(kind, ss.sig.p, 0), ss.ml.p, 1, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(tl_ctx->join[0], st));
    return BLSMI_OK;
}
int aggregate_tail(const i32* d_prod, const SigSide& ss, int* ok) {
    HIPCHK(hipStreamWaitEvent(g_stream, tl_ctx->join[0], 0));
    return tail_verdict(LAT_AGGTAIL2_OFFSET, {.b2 = {ss.ml.p, 0}, .b3 = {d_prod, 0}}, ok);
}
inline bool sig_is_infinity(int kind, const uint8_t* sig, int fmt) {       // the reference panics in MillerLoop: verdict 0
    const Kind k = kind_of(kind);
    return (fmt & FMT_SIG_JAC) ? jac_host_is_infinity(sig, k.sig_bytes) : all_zero(sig, k.sig_bytes);
}
// below this many messages the duplicate screen runs inline on the calling thread (a few microseconds) before any GPU work
constexpr size_t DUP_INLINE_MAX = 4096;
// The tuple side of an unsplit VerifyAggregate as the leased context's device sees it: messages, offsets (kind 2: the domain) and keys (or
// prep: their tables) at device addresses.  The device-pointer forms have them there.  The host form stages them through its two hooks:
// stage_msgs, before the duplicate screen and the hash, takes the buffers, fills in the three addresses and enqueues the copy of the
// messages and offsets; after_hash (the keys) runs once the hash is enqueued, as aggregate_shard_dev's.  msgs / off: the host's own copy of
// the messages where the caller passed one (the duplicate screen's sort fallback reads it; otherwise it fetches them from the device).
struct AggInputs {
    const void* d_msgs = nullptr; const void* d_off_or_domain = nullptr; const u8* d_pks = nullptr; const PrepKeys* prep = nullptr;
    const uint8_t* msgs = nullptr; const uint64_t* off = nullptr;
    std::function<int(AggInputs&)> stage_msgs;
    std::function<int()> after_hash;
};
// the duplicate verdict of the reference's sort (has_duplicates_sorted) where the device table gave up (k_util.hip), or "dup_force_sort" asks
int dup_sort_fallback(const AggInputs& in, size_t n, bool* dup) {
    try {
        if (in.msgs) { *dup = has_duplicates_sorted(in.msgs, in.off, n); return BLSMI_OK; }
        std::vector<uint64_t> off(n + 1);                                  // resident messages: fetched
        HIPCHK(hipMemcpyAsync(off.data(), in.d_off_or_domain, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, g_stream)); HIPCHK(hipStreamSynchronize(g_stream));
        std::vector<uint8_t> m((size_t)off[n] ? (size_t)off[n] : 1);
        HIPCHK(hipMemcpyAsync(m.data(), in.d_msgs, (size_t)off[n], hipMemcpyDeviceToHost, g_stream)); HIPCHK(hipStreamSynchronize(g_stream));
        *dup = has_duplicates_sorted(m.data(), off.data(), n);
        return BLSMI_OK;
    } catch (...) { return BLSMI_E_NOMEM; }
}
// An unsplit VerifyAggregate on the leased context -- the host form's one-shard case and every device-pointer form.  in: by value, the
// host form's stage_msgs completes it.  sig: host memory,
// not the point at infinity; *ok is 0 on entry.  screen: the duplicate-message rule of g2pubs/bls.go:245-261 is still to be applied, on the
// device (k_util.hip).  Enqueue order: the signature side on aux[0]; the message copy; the duplicate screen; the hash; the key upload or the
// prepared gather; the infinity flags; the Miller loops; the product tree; then the flag fetches.  A repeated or empty message ends the
// call as a key at infinity does (bad bit 0: verdict 0; the lease drains the side stream).
int verify_aggregate_on_ctx(int kind, AggInputs in, const uint8_t* sig, size_t n, int* ok, bool screen, int fmt) {
    screen = screen && kind != 2 && n > 0;
    DBuf prod, ddup; HIPCHK(prod.alloc(sizeof(i32) * 12 * NL)); HIPCHK(ddup.alloc(sizeof(int)));
    SigSide ss;
    { int rc = sig_side_start(kind, sig, ss, fmt); if (rc) return rc; }
    if (n == 0) launch_quiet(KERNEL_OF(k_fq12_one), 1, g_stream, prod.p);
    else {
        bool first = true;
        int bad = 0;
        int rc = tuple_side_product(agg_pow_wanted(kind, n, tune()), prod, &bad, [&](bool g1_clear, int* b) -> int {
            const bool fresh = first;                                      // (the second run: messages, keys and the screen's verdict are where the first left them)
            first = false;
            if (fresh && in.stage_msgs) { int rc = in.stage_msgs(in); if (rc) return rc; }
            if (fresh && screen && blsmi_util::dup_check_async(in.d_msgs, in.d_off_or_domain, n, dup_key()[0], dup_key()[1], ddup.as<int>(), g_stream, [](size_t b) { return tl_ctx->arena.alloc(b); }) != 0) return BLSMI_E_HIP;
            int rc = aggregate_shard_dev(kind, in.d_msgs, in.d_off_or_domain, in.d_pks, n, prod.as<i32>(), b, g_stream, fresh ? in.after_hash : std::function<int()>{}, in.prep, g1_clear);
            if (rc) return rc;
            HIPCHK(hipStreamSynchronize(g_stream));
            if (!fresh || !screen) return BLSMI_OK;
            int dupflag = 0;
            HIPCHK(hipMemcpyAsync(&dupflag, ddup.p, sizeof dupflag, hipMemcpyDeviceToHost, g_stream)); HIPCHK(hipStreamSynchronize(g_stream));
            if (tune().dup_force_sort) dupflag |= 2;                       // test hook: take the fallback on every call
            if (dupflag & 2) { bool d = false; rc = dup_sort_fallback(in, n, &d); if (rc) return rc; dupflag = d ? 1 : 0; }
            if (dupflag) *b |= 1;
            return BLSMI_OK;
        });
        if (rc || bad) return rc;                                          // a key at infinity / a repeated or empty message: verdict 0
    }
    return aggregate_tail(prod.as<i32>(), ss, ok);
}
// e(sig-side) == prod_i e(h_i, pk_i): n Miller loops, an Fq12 product tree, ONE final exponentiation
// (FinalExponentiation is a homomorphism, so the verdict equals the reference's product of n full pairings).
// A call that is not split (one shard; the common case of a small aggregate and of a single-device deployment) runs on
// ANY free context of any device, holds no process-wide lock and touches no other device: concurrent VerifyAggregate
// calls from several goroutines run side by side on the library's streams.  A call that IS split occupies every
// device anyway: it takes g_coll_mu, each shard leaves its partial product in its device's exchange buffer, one
// all-gather (720 bytes per slot) brings them together, device 0 multiplies them and compares.
int verify_aggregate_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, const uint8_t* sig, size_t n, int* ok, bool check_dups, int fmt = 0) {
    if (!ok || !sig || (n && (!msgs || !off_or_domain || !pks))) return BLSMI_E_ARG;
    *ok = 0;
    { std::lock_guard<std::mutex> lk(g_mu); int rc = ensure_init_default(); if (rc) return rc; }
    const Kind k = kind_of(kind);
    if (sig_is_infinity(kind, sig, fmt)) return BLSMI_OK;
    const size_t pk_in = rec_bytes(k.pk_bytes, fmt & FMT_PK_JAC);
    const size_t words = (size_t)12 * NL;
    const ShardPlan plan = plan_shards(n, 64);
    const Tuning t = tuning_now();                                         // what holds across the shards' threads is decided here, once
    check_dups = check_dups && n > 0;
    bool dup = false;
    if (check_dups && n <= DUP_INLINE_MAX) {                               // small: screened here, no thread, no device work
        int rc = has_duplicates_rc(msgs, off_or_domain, n, &dup, t.dup_force_sort);
        if (rc) return rc;
        if (dup) return BLSMI_OK;
        check_dups = false;
    }
    if (plan.nshards == 1 && !g_force_rccl) {
        CtxLease lease;                                                    // any device, any free context
        if (lease.rc) return lease.rc;
        if (n == 0) return verify_aggregate_on_ctx(kind, AggInputs{}, sig, 0, ok, false, fmt);
        DevMsgs dm(kind, off_or_domain, n); DBuf dp;
        AggInputs in;
        in.msgs = msgs; in.off = off_or_domain;
        in.stage_msgs = [&](AggInputs& a) -> int {
            int rc = dm.alloc(); if (rc) return rc;
            HIPCHK(dp.alloc((size_t)k.pk_bytes * n));
            a.d_msgs = dm.m.p; a.d_off_or_domain = dm.off.p; a.d_pks = dp.as<u8>();
            return dm.copy(msgs, off_or_domain, g_stream);
        };
        in.after_hash = [&]() -> int { return upload_points(k.pk(), (fmt & FMT_PK_JAC) != 0, pks, dp.p, n, g_stream); };   // the hash runs while the keys are on their way (in-memory points: + ToAffine on the device)
        return verify_aggregate_on_ctx(kind, in, sig, n, ok, check_dups, fmt);
    }
    const int S = (plan.nshards + g_ndev - 1) / g_ndev;                    // partial-product slots per device
    const size_t total = (size_t)g_ndev * S;
    std::unique_lock<std::mutex> coll_lk(g_coll_mu);
    // exchange buffer of every device, in 180-word records: [0, S) this device's slots | [S, S + total) gathered |
    // then on device 0: one spare record | SoA copy of the gathered records | product-tree scratch
    int rc = coll_reserve_all(sizeof(i32) * words * (S + 3 * total + 4), false);
    if (rc) return rc;
    for (int d = 0; d < g_ndev; d++) {                                       // slots start as 1 (a shard with no tuples contributes nothing)
        HIPCHK(hipSetDevice(g_dev[d].id));
        for (int sl = 0; sl < S; sl++) launch_quiet(KERNEL_OF(k_fq12_one), 1, g_dev[d].coll_stream, reinterpret_cast<i32*>(g_dev[d].coll.p) + words * sl);
    }
    rc = coll_sync_all();
    if (rc) return rc;
    i32* c0 = reinterpret_cast<i32*>(g_dev[0].coll.p);
    i32* lhs = c0 + words * (S + total);                                   // spare record
    // the messages of a split call are spread over the devices: the duplicate screen runs on the host beside the shards
    int dup_rc = BLSMI_OK;
    std::thread dup_thread;
    if (check_dups) {
        try { dup_thread = std::thread([&] { dup_rc = has_duplicates_rc(msgs, off_or_domain, n, &dup, t.dup_force_sort); }); }
        catch (...) { dup_rc = has_duplicates_rc(msgs, off_or_domain, n, &dup, t.dup_force_sort); }   // no thread to be had: screen here
    }
    bool powc = agg_pow_wanted(kind, n, t);                                // hash points without their cofactor clearing, the product raised to 1 - x instead
    int bad = 0;
    rc = BLSMI_OK;
    if (n) rc = run_tuple_side(powc, &bad, [&](bool g1_clear, int* any_bad) -> int {
        std::vector<int> shard_bad(plan.nshards, 0);
        auto shard_body = [&](int sh, size_t lo, size_t hi) -> int {
            const size_t m = hi - lo;
            std::vector<uint64_t> off_sub;
            const uint8_t* mp; const uint64_t* op;
            if (kind == 2) { mp = msgs + 32 * lo; op = off_or_domain; }
            else {
                off_sub.resize(m + 1);
                for (size_t i = 0; i <= m; i++) off_sub[i] = off_or_domain[lo + i] - off_or_domain[lo];
                mp = msgs + off_or_domain[lo]; op = off_sub.data();
            }
            i32* slot = reinterpret_cast<i32*>(tl_ctx->dev->coll.p) + words * (sh / g_ndev);
            return aggregate_shard(kind, mp, op, pks + pk_in * lo, m, slot, &shard_bad[sh], g1_clear, fmt);
        };
        int rc;
        if (plan.nshards == 1) { CtxLease lease(0); rc = lease.rc ? lease.rc : shard_body(0, 0, n); }   // (forced RCCL with one shard: test hook)
        else rc = run_shards(plan, shard_body);
        for (int b : shard_bad) *any_bad |= b;
        return rc;
    });
    if (dup_thread.joinable()) dup_thread.join();
    if (rc) return rc;
    if (dup_rc) return dup_rc;
    if ((bad & 1) || dup) return BLSMI_OK;                                 // a key at infinity / a repeated or empty message: *ok stays 0
    // the one exchange step of VerifyAggregate: all-gather of the per-device partial products
    const i32* gathered = c0; size_t cnt = S;
    if (g_have_comm && g_alias) {
        rc = alias_allgather(sizeof(i32) * words * S);
        if (rc) return rc;
        gathered = c0 + words * S; cnt = total;
    } else if (g_have_comm) {
        NCCLCHK(g_rccl.GroupStart());
        for (int d = 0; d < g_ndev; d++) {
            i32* base = reinterpret_cast<i32*>(g_dev[d].coll.p);
            NCCLCHK(g_rccl.AllGather(base, base + words * S, words * S, ncclInt32, g_dev[d].comm, g_dev[d].coll_stream));
        }
        NCCLCHK(g_rccl.GroupEnd());
        rc = coll_sync_all();
        if (rc) return rc;
        gathered = c0 + words * S; cnt = total;
    }
    CtxLease lease(0);
    if (lease.rc) return lease.rc;
    i32* soa = lhs + words; i32* scratch = soa + words * total;
    launch_quiet(KERNEL_OF(k_fq12_aos_to_soa), nblocks(words * cnt), g_stream, gathered, soa, cnt);
    const i32* src = prod_tree(soa, cnt, scratch, soa, g_stream);
    if (powc) { i32* dst = src == soa ? scratch : soa; int rc2 = aggregate_pow_c(src, dst); if (rc2) return rc2; src = dst; }   // (dst: the tree's other buffer, free now)
    return aggregate_tail(kind, src, sig, ok, fmt);
}
// Device-pointer forms: messages, offsets and keys (or their prepared tables) resident on ONE of the library's devices, whose lease the
// caller holds; the aggregate signature is 96 / 192 bytes of HOST memory.  Duplicate rejection runs on the device (k_util.hip).  Not split
// over devices: the caller's buffers live on one.
int verify_aggregate_dev(int kind, const void* d_msgs, const void* d_off_or_domain, const void* d_pks, const uint8_t* sig, size_t n, int* ok, bool check_dups, const PrepKeys* prep = nullptr, int fmt = 0) {
    *ok = 0;
    if (sig_is_infinity(kind, sig, fmt)) return BLSMI_OK;
    return verify_aggregate_on_ctx(kind, AggInputs{d_msgs, d_off_or_domain, (const u8*)d_pks, prep}, sig, n, ok, check_dups, fmt);
}

// VerifyAggregateCommon: AggregatePublicKeys (sum) then one Verify (g2pubs/bls.go:275-278)
// fmt (blsmi.hip: FMT_*): bit 0 -- d_pks / pks are in-memory Jacobian records (summed as they are: k_g?_sum0_jac), bit 1 -- so is the signature
int verify_aggregate_common_dev(int kind, const void* d_pks, size_t n, const uint8_t* msg, size_t msg_len, const uint8_t* domain, const uint8_t* sig, int* ok, int fmt = 0);
constexpr size_t COMMON_ONE_LEASE_MAX = (size_t)1 << 17;                   // above: the sum is split over the devices (blsmi_g?_sum) and dominates anyway
int verify_aggregate_common_host(int kind, const uint8_t* msg, size_t msg_len, const uint8_t* domain, const uint8_t* pks, const uint8_t* sig, size_t n, int* ok, int fmt = 0) {
    if (!ok || !sig || !msg || (n && !pks)) return BLSMI_E_ARG;
    const Kind k = kind_of(kind);
    const size_t pk_in = rec_bytes(k.pk_bytes, fmt & FMT_PK_JAC);
    if (n > 0 && n <= COMMON_ONE_LEASE_MAX) {                              // one context: the key sum runs beside the hash (verify_aggregate_common_dev)
        { std::lock_guard<std::mutex> lk(g_mu); int rc0 = ensure_init_default(); if (rc0) return rc0; }
        CtxLease lease;
        if (lease.rc) return lease.rc;
        DBuf dp; HIPCHK(dp.alloc(pk_in * n));
        HIPCHK(hipMemcpyAsync(dp.p, pks, pk_in * n, hipMemcpyHostToDevice, g_stream));
        return verify_aggregate_common_dev(kind, dp.p, n, msg, msg_len, domain, sig, ok, fmt);
    }
    uint8_t agg[192]; int agg_inf = 0;
    int rc = sum_host(k.pk_group, pks, nullptr, n, agg, &agg_inf, (fmt & FMT_PK_JAC) != 0);
    if (rc) return rc;
    uint8_t flags = agg_inf ? 1 : 0, res = 0;
    if (kind == 2) rc = verify_batch_host(2, msg, reinterpret_cast<const uint64_t*>(domain), agg, sig, &flags, &res, nullptr, 1, fmt & FMT_SIG_JAC);
    else { const uint64_t off[2] = {0, (uint64_t)msg_len}; rc = verify_batch_host(kind, msg, off, agg, sig, &flags, &res, nullptr, 1, fmt & FMT_SIG_JAC); }
    *ok = res;
    return rc;
}
// The same with the n public keys RESIDENT on one of the library's devices (a validator set kept in HBM): tree sum where they lie,
// then one Verify; message, domain and signature are a few host bytes.  The caller holds the lease of the keys' device.
int verify_aggregate_common_dev(int kind, const void* d_pks, size_t n, const uint8_t* msg, size_t msg_len, const uint8_t* domain, const uint8_t* sig, int* ok, int fmt) {
    const Kind k = kind_of(kind);
    const bool pj = (fmt & FMT_PK_JAC) != 0;
    *ok = 0;
    DBuf dagg, dflag, dm, doff, dsig, dinf, dok;
    HIPCHK(dagg.alloc(k.pk_bytes)); HIPCHK(dflag.alloc(sizeof(i32))); HIPCHK(dm.alloc(msg_len ? msg_len : 1)); HIPCHK(doff.alloc(16));
    HIPCHK(dsig.alloc(k.sig_bytes)); HIPCHK(dinf.alloc(1)); HIPCHK(dok.alloc(1));
    // AggregatePublicKeys does not depend on the message: the tree sum runs on a side stream WHILE the message is hashed (and the signature
    // side's Miller loop on the other one, verify_sig_side_start); its infinity flag travels on the device.  The pair stage waits for it.
    HIPCHK(tl_ctx->ensure_aux());
    hipStream_t side = tl_ctx->aux[1];
    HIPCHK(hipEventRecord(tl_ctx->fork, g_stream)); HIPCHK(hipStreamWaitEvent(side, tl_ctx->fork, 0));   // (the caller's stream may still be producing the keys)
    if (n == 0) {                                                          // the empty sum is the point at infinity (g2pubs/bls.go:181)
        HIPCHK(hipMemsetAsync(dagg.p, 0, k.pk_bytes, side)); HIPCHK(hipMemsetAsync(dinf.p, 1, 1, side));
    } else {
        int rc = sum_dev(k.pk(), (const u8*)d_pks, (const u8*)nullptr, n, dagg.as<u8>(), dflag.as<i32>(), side, false, pj);
        if (rc) return rc;
        launch_quiet(KERNEL_OF(k_flag_to_byte), 1, side, dflag.p, dinf.p);
    }
    HIPCHK(hipEventRecord(tl_ctx->join[1], side));
    uint64_t off[2] = {0, (uint64_t)msg_len};
    if (msg_len) HIPCHK(hipMemcpyAsync(dm.p, msg, msg_len, hipMemcpyHostToDevice, g_stream));
    if (kind == 2) HIPCHK(hipMemcpyAsync(doff.p, domain, 8, hipMemcpyHostToDevice, g_stream));
    else HIPCHK(hipMemcpyAsync(doff.p, off, sizeof off, hipMemcpyHostToDevice, g_stream));
    { int rc = upload_points(k.sig(), (fmt & FMT_SIG_JAC) != 0, sig, dsig.p, 1, g_stream); if (rc) return rc; }
    int rc = verify_batch_dev(kind, dm.p, doff.p, dagg.p, dsig.p, dinf.p, dok.p, 1, g_stream, nullptr, tl_ctx->join[1]);   // synchronises
    if (rc) return rc;
    uint8_t res = 0;
    HIPCHK(hipMemcpyAsync(&res, dok.p, 1, hipMemcpyDeviceToHost, g_stream)); HIPCHK(hipStreamSynchronize(g_stream));
    *ok = res;
    return BLSMI_OK;
}
int hash_host(int kernel_kind, const uint8_t* msgs, const void* off_or_domain, uint8_t* out, size_t n) {
    if (n && (!msgs || !off_or_domain || !out)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    const size_t OB = kind_of(kernel_kind).h_bytes;
    DevMsgs dm(kernel_kind, off_or_domain, n); DBuf dout;
    HIPCHK(dout.alloc(OB * n));
    int rc = dm.upload(msgs, off_or_domain, g_stream);
    if (rc) return rc;
    rc = hash_dev(kernel_kind, dm.m.p, dm.off.p, dout.as<u8>(), n, g_stream, hash_route_alone(kernel_kind, n));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, OB * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// n compressed points -> affine records, infinity flags, error codes (g1.go:185-249, g2.go:219-295), on stream s.
// Small batches take the subgroup test (check == 1) as a level program of the latency path.
int decompress_dev(const GroupKernels& gk, const u8* d_in, int check, u8* d_out, u8* d_inf, u8* d_err, size_t n, hipStream_t s) {
    const unsigned g = nblocks(n);
    const bool lat = check == 1 && n <= tune().lat_max;
    const int kcheck = lat ? 0 : check;
    const size_t wave_max = tune().swu_wave_max;
    const bool waves = kcheck == 0 && n <= wave_max;                       // the smallest calls: one wave per point, its square root with one limb per lane (fp_row.cuh)
    if (waves) launch_sized(gk.decompress_waves, n, 64, s, d_in, d_out, d_inf, d_err, n);
    else launch(gk.decompress, g, s, d_in, kcheck, d_out, d_inf, d_err, n);
    if (lat) {
        DBuf sub; HIPCHK(sub.alloc(n, s));
        launch_lat_marked(gk.lat_subgrp, s, {.b0 = {d_out, gk.wire_bytes}, .ok = sub.p}, n);
        launch_quiet(KERNEL_OF(k_apply_subgroup), g, s, sub.p, d_out, (int)(gk.wire_bytes / 4), d_inf, d_err, n);
    }
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
int decompress_host(int group, const uint8_t* in, int check, uint8_t* out, uint8_t* out_inf, uint8_t* err, size_t n) {
    if (n && (!in || !out || !out_inf || !err)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    const GroupKernels& gk = group_kernels(group);
    const size_t OB = gk.wire_bytes, IB = OB / 2;
    DBuf di, dout, dinf, derr;
    HIPCHK(di.alloc(IB * n)); HIPCHK(dout.alloc(OB * n)); HIPCHK(dinf.alloc(n)); HIPCHK(derr.alloc(n));
    HIPCHK(hipMemcpyAsync(di.p, in, IB * n, hipMemcpyHostToDevice, g_stream));
    { const int rc = decompress_dev(gk, di.as<u8>(), check, dout.as<u8>(), dinf.as<u8>(), derr.as<u8>(), n, g_stream); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(out, dout.p, OB * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(out_inf, dinf.p, n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(err, derr.p, n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// Deserialize + Verify in one device pass: compressed keys and signatures (what Serialize() produces and real callers
// hold, g1.go:185-249, g2.go:219-289) are decompressed -- with the subgroup check when `check` is set, as
// DeserializePublicKey / DeserializeSignature do -- and verified without the affine forms visiting the host.
// A tuple whose key or signature fails to deserialise, or is the point at infinity, gets verdict 0; the
// per-element error codes of blsmi_g{1,2}_decompress_batch are returned when asked for.
int verify_serialized_host(int kind, const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, int check,
                           uint8_t* ok, uint8_t* err_pk, uint8_t* err_sig, size_t n) {
    if (n && (!msgs || !off || !pks || !sigs || !ok)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    const Kind k = kind_of(kind);
    const size_t pkc = k.pk_bytes / 2, sgc = k.sig_bytes / 2;
    DevMsgs dm(kind, off, n); DBuf dpc, dsc, dp, ds, ipk, epk, isg, esg, dfl, dok;
    HIPCHK(dpc.alloc(pkc * n)); HIPCHK(dsc.alloc(sgc * n)); HIPCHK(dp.alloc((size_t)k.pk_bytes * n)); HIPCHK(ds.alloc((size_t)k.sig_bytes * n));
    HIPCHK(ipk.alloc(n)); HIPCHK(epk.alloc(n)); HIPCHK(isg.alloc(n)); HIPCHK(esg.alloc(n)); HIPCHK(dfl.alloc(n)); HIPCHK(dok.alloc(n));
    { int rc = dm.upload(msgs, off, g_stream); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(dpc.p, pks, pkc * n, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dsc.p, sigs, sgc * n, hipMemcpyHostToDevice, g_stream));
    const unsigned g = nblocks(n);
    // The two decompressions and the hash are independent, each a serial chain per lane: for a small call they go to three
    // streams (fork after the input copies, join before the pairing stage) -- 8.7 -> ~5 ms for one tuple.  So do batches up to
    // 131 072 tuples: their one-lane kernels put one or two waves on a SIMD and the kernels with 256 registers a lane share it
    // (BLSMI_SIDE_MAX; a larger batch fills the chip by itself and stays on one stream).
    const size_t side_max = tune().side_max;
    const bool side = n <= std::max(tune().lat_max, side_max);
    hipStream_t spk = g_stream, ssg = g_stream;
    if (side) {
        HIPCHK(tl_ctx->ensure_aux());
        HIPCHK(hipEventRecord(tl_ctx->fork, g_stream));
        spk = tl_ctx->aux[0]; ssg = tl_ctx->aux[1];
        HIPCHK(hipStreamWaitEvent(spk, tl_ctx->fork, 0)); HIPCHK(hipStreamWaitEvent(ssg, tl_ctx->fork, 0));
    }
    {
        int rc = decompress_dev(k.pk(), dpc.as<u8>(), check, dp.as<u8>(), ipk.as<u8>(), epk.as<u8>(), n, spk);
        if (rc) return rc;
        rc = decompress_dev(k.sig(), dsc.as<u8>(), check, ds.as<u8>(), isg.as<u8>(), esg.as<u8>(), n, ssg);
        if (rc) return rc;
    }
    DBuf h, f;
    HIPCHK(h.alloc((size_t)k.h_bytes * n)); HIPCHK(f.alloc(sizeof(i32) * 12 * NL * n));
    const VerifyRoute r = verify_route(kind, n, false, false, tune(), route_load(n));   // (no signature side: the signatures are still being decompressed)
    int rc = hash_dev(kind, dm.m.p, dm.off.p, h.as<u8>(), n, g_stream, r.hash);  // on the main stream, beside the decompressions
    if (rc) return rc;
    if (side) {
        HIPCHK(hipEventRecord(tl_ctx->join[0], spk)); HIPCHK(hipEventRecord(tl_ctx->join[1], ssg));
        HIPCHK(hipStreamWaitEvent(g_stream, tl_ctx->join[0], 0)); HIPCHK(hipStreamWaitEvent(g_stream, tl_ctx->join[1], 0));
    }
    launch_quiet(KERNEL_OF(k_merge_flags), g, g_stream, ipk.p, epk.p, isg.p, esg.p, dfl.p, n);
    HIPCHK(hipGetLastError());
    rc = verify_pair_stage(kind, h.as<u8>(), dp.p, ds.p, dfl.p, dok.p, f.as<i32>(), n, g_stream, r);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ok, dok.p, n, hipMemcpyDeviceToHost, g_stream));
    if (err_pk) HIPCHK(hipMemcpyAsync(err_pk, epk.p, n, hipMemcpyDeviceToHost, g_stream));
    if (err_sig) HIPCHK(hipMemcpyAsync(err_sig, esg.p, n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// Point validation (blsmi 0.14): the status byte of n points as they arrive -- affine wire records (+ optional infinity flags) or, jac, the
// reference's in-memory Jacobian records -- in ONE launch for every n (k_check.hip).  check: 0 / 1 / 2 as decompress_dev.  Reads only.
int check_dev(const GroupKernels& gk, bool jac, const void* d_pts, const void* d_in_inf, int check, void* d_status, size_t n, hipStream_t s) {
    if (jac) launch_items(gk.check_jac, n, s, d_pts, check, d_status, n);
    else launch_items(gk.check, n, s, d_pts, d_in_inf, check, d_status, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
inline int check_args(const void* pts, const void* status, int check, size_t n) {   // what both forms refuse before any device work
    if (check < 0 || check > 2) return BLSMI_E_ARG;
    if (n && (!pts || !status)) return BLSMI_E_ARG;
    return BLSMI_OK;
}
int check_host(int group, bool jac, const uint8_t* pts, const uint8_t* in_inf, int check, uint8_t* status, size_t n) {
    { const int rc = check_args(pts, status, check, n); if (rc) return rc; }
    if (n == 0) return BLSMI_OK;
    LOCK_AND_INIT();
    const GroupKernels& gk = group_kernels(group);
    const size_t IB = rec_bytes(gk.wire_bytes, jac);
    const bool flags = in_inf && !jac;
    DBuf di, dinf, dst;
    HIPCHK(di.alloc(IB * n)); HIPCHK(dinf.alloc(n)); HIPCHK(dst.alloc(n));
    HIPCHK(hipMemcpyAsync(di.p, pts, IB * n, hipMemcpyHostToDevice, g_stream));
    if (flags) HIPCHK(hipMemcpyAsync(dinf.p, in_inf, n, hipMemcpyHostToDevice, g_stream));
    { const int rc = check_dev(gk, jac, di.p, flags ? dinf.p : nullptr, check, dst.p, n, g_stream); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(status, dst.p, n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
int check_dev_api(int group, const void* d_pts, const void* d_in_inf, int jac, int check, void* d_status, size_t n, void* stream) {
    { const int rc = check_args(d_pts, d_status, check, n); if (rc) return rc; }
    if (jac && d_in_inf) return BLSMI_E_ARG;
    if (n == 0) return BLSMI_OK;
    LOCK_AND_INIT_AT(d_status);
    UseStream us(stream);
    { const int rc = check_dev(group_kernels(group), jac != 0, d_pts, d_in_inf, check, d_status, n, g_stream); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
int compress_host(int group, const uint8_t* pts, const uint8_t* in_inf, uint8_t* out, size_t n) {
    if (n && (!pts || !out)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    const GroupKernels& gk = group_kernels(group);
    const size_t IB = gk.wire_bytes, OB = IB / 2;
    DBuf di, dinf, dout;
    HIPCHK(di.alloc(IB * n)); HIPCHK(dinf.alloc(n)); HIPCHK(dout.alloc(OB * n));
    HIPCHK(hipMemcpyAsync(di.p, pts, IB * n, hipMemcpyHostToDevice, g_stream));
    if (in_inf) HIPCHK(hipMemcpyAsync(dinf.p, in_inf, n, hipMemcpyHostToDevice, g_stream));
    launch_quiet(gk.compress, nblocks(n), g_stream, di.p, in_inf ? dinf.p : nullptr, dout.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, OB * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// The wire format <-> the reference's in-memory points (blsmi 0.15).  Decompression: what decompress_dev gives for the same bytes and check,
// its records as store_jac_m384 writes them -- (x, y, 1), and (0, 1, 0) wherever the affine record is the all-zero one (a well-formed infinity,
// every err != 0).  The calls decompress_dev serves with the one-lane kernel take its twin that writes the in-memory record itself; the small
// calls it serves otherwise (a wave per point, the subgroup test as a level program) run unchanged into a temporary and k_affine_to_jac
// finishes, reading the all-zero record as every kernel does.  d_inf may be null.  The bytes are the same on every route.
int decompress_jac_dev(const GroupKernels& gk, const u8* d_in, int check, u64* d_out, u8* d_inf, u8* d_err, size_t n, hipStream_t s) {
    const bool lat = check == 1 && n <= tune().lat_max;
    const bool waves = (lat ? 0 : check) == 0 && n <= tune().swu_wave_max;
    if (!lat && !waves) {
        launch(gk.decompress_jac, nblocks(n), s, d_in, check, d_out, d_inf, d_err, n);
        prof_mark(nullptr);
        HIPCHK(hipGetLastError());
        return BLSMI_OK;
    }
    DBuf aff, inf;
    HIPCHK(aff.alloc(gk.wire_bytes * n, s)); HIPCHK(inf.alloc(n, s));
    u8* flags = d_inf ? d_inf : inf.as<u8>();
    { const int rc = decompress_dev(gk, d_in, check, aff.as<u8>(), flags, d_err, n, s); if (rc) return rc; }
    launch(KERNEL_OF(k_affine_to_jac), nblocks(n), s, aff.p, nullptr, 1, gk.id, d_out, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
inline int decompress_jac_args(const void* in, const void* out, const void* err, int check, size_t n) {   // what both forms refuse before any device work
    if (check < 0 || check > 2) return BLSMI_E_ARG;
    if (n && (!in || !out || !err)) return BLSMI_E_ARG;
    return BLSMI_OK;
}
int decompress_jac_host(int group, const uint8_t* in, int check, uint64_t* out, uint8_t* out_inf, uint8_t* err, size_t n) {
    { const int rc = decompress_jac_args(in, out, err, check, n); if (rc) return rc; }
    if (n == 0) return BLSMI_OK;
    LOCK_AND_INIT();
    const GroupKernels& gk = group_kernels(group);
    const size_t IB = gk.wire_bytes / 2, OB = rec_bytes(gk.wire_bytes, true);
    DBuf di, dout, dinf, derr;
    HIPCHK(di.alloc(IB * n)); HIPCHK(dout.alloc(OB * n)); HIPCHK(dinf.alloc(n)); HIPCHK(derr.alloc(n));
    HIPCHK(hipMemcpyAsync(di.p, in, IB * n, hipMemcpyHostToDevice, g_stream));
    { const int rc = decompress_jac_dev(gk, di.as<u8>(), check, dout.as<u64>(), out_inf ? dinf.as<u8>() : nullptr, derr.as<u8>(), n, g_stream); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(out, dout.p, OB * n, hipMemcpyDeviceToHost, g_stream));
    if (out_inf) HIPCHK(hipMemcpyAsync(out_inf, dinf.p, n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(err, derr.p, n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
int decompress_jac_dev_api(int group, const void* d_in, int check, void* d_out, void* d_inf, void* d_err, size_t n, void* stream) {
    { const int rc = decompress_jac_args(d_in, d_out, d_err, check, n); if (rc) return rc; }
    if (n == 0) return BLSMI_OK;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    { const int rc = decompress_jac_dev(group_kernels(group), static_cast<const u8*>(d_in), check, static_cast<u64*>(d_out), static_cast<u8*>(d_inf), static_cast<u8*>(d_err), n, g_stream); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// Compression: the bytes compress_host gives for the record and flag jac_to_wire_dev gives, in ONE launch for every n and without the affine
// records in between (k_g?_compress_jac, one lane per point).  Reads only.
int compress_jac_dev(const GroupKernels& gk, const void* d_jac, void* d_out, size_t n, hipStream_t s) {
    launch(gk.compress_jac, nblocks(n), s, d_jac, d_out, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
int compress_jac_host(int group, const uint64_t* jac, uint8_t* out, size_t n) {
    if (n && (!jac || !out)) return BLSMI_E_ARG;
    if (n == 0) return BLSMI_OK;
    LOCK_AND_INIT();
    const GroupKernels& gk = group_kernels(group);
    const size_t IB = rec_bytes(gk.wire_bytes, true), OB = gk.wire_bytes / 2;
    DBuf di, dout;
    HIPCHK(di.alloc(IB * n)); HIPCHK(dout.alloc(OB * n));
    HIPCHK(hipMemcpyAsync(di.p, jac, IB * n, hipMemcpyHostToDevice, g_stream));
    { const int rc = compress_jac_dev(gk, di.p, dout.p, n, g_stream); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(out, dout.p, OB * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
int compress_jac_dev_api(int group, const void* d_jac, void* d_out, size_t n, void* stream) {
    if (n && (!d_jac || !d_out)) return BLSMI_E_ARG;
    if (n == 0) return BLSMI_OK;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    { const int rc = compress_jac_dev(group_kernels(group), d_jac, d_out, n, g_stream); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
}  // namespace

// Shard-level half of VerifyAggregate for callers that shard ACROSS PROCESSES (one rank per GPU under torchrun, bls_amd/dist.py):
// prod_i MillerLoop(H(m_i), pk_i) over this rank's n tuples (no final exponentiation), returned in the Fq12 wire format.
// n == 0 gives 1.  *bad (may be null) = 1 when some key is the point at infinity (all-zero record).
static int aggregate_partial_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, size_t n, uint64_t* out72, int* bad) {
    if (!out72 || (n && (!msgs || !off_or_domain || !pks))) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    const size_t words = (size_t)12 * NL;
    DBuf dout, f; HIPCHK(dout.alloc(576)); HIPCHK(f.alloc(sizeof(i32) * words));
    int b = 0;
    if (n == 0) launch_quiet(KERNEL_OF(k_fq12_one), 1, g_stream, f.p);
    else {
        // a large g2pubs shard pairs the hash points before their cofactor clearing and raises ITS product to 1 - x (agg_pow_wanted): the
        // value differs from prod ML(H(m_i), pk_i) only by what the final exponentiation removes, which is all a partial product is used for
        int rc = tuple_side_product(agg_pow_wanted(kind, n, tune()), f, &b, [&](bool g1_clear, int* bad) { return aggregate_shard(kind, msgs, off_or_domain, pks, n, f.as<i32>(), bad, g1_clear); });
        if (rc) return rc;
    }
    launch_quiet(KERNEL_OF(k_final_exp), 1, g_stream, f.p, dout.p, 1, 1);   // mode 1: format conversion only
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out72, dout.p, 576, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    if (bad) *bad = b & 1;
    return BLSMI_OK;
}
BLSMI_API int blsmi_g2pubs_aggregate_partial(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, size_t n, uint64_t* out72, int* bad) { return aggregate_partial_host(0, msgs, off, pks, n, out72, bad); }
BLSMI_API int blsmi_g1pubs_aggregate_partial(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, size_t n, uint64_t* out72, int* bad) { return aggregate_partial_host(1, msgs, off, pks, n, out72, bad); }
// product of n Fq12 values in the wire format (tree on the device)
BLSMI_API int blsmi_fq12_product(const uint64_t* in, size_t n, uint64_t* out72) {
    if (!out72 || !in || n == 0) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    const size_t words = (size_t)12 * NL;
    DBuf di, fr0, fr1, dout;
    HIPCHK(di.alloc(576 * n)); HIPCHK(fr0.alloc(sizeof(i32) * words * n)); HIPCHK(fr1.alloc(sizeof(i32) * words * ((n + 1) / 2))); HIPCHK(dout.alloc(576));
    HIPCHK(hipMemcpyAsync(di.p, in, 576 * n, hipMemcpyHostToDevice, g_stream));
    launch_quiet(KERNEL_OF(k_fq12_from_m384), nblocks(n), g_stream, di.p, fr0.p, n);
    const i32* src = prod_tree(fr0.as<i32>(), n, fr1.as<i32>(), fr0.as<i32>(), g_stream);
    launch_quiet(KERNEL_OF(k_final_exp), 1, g_stream, src, dout.p, 1, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out72, dout.p, 576, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}

// ---- the two halves behind the small-batch hashes, exported for the parity tests ------------------------------------------
// kind 0 / 1 / 2 = HashG1 / HashG2 / HashG2WithDomain.  pts: n records of the mapped points (kind 0: 2 G1 points = 192 bytes,
// kind 1: 2 G2 points = 384, kind 2: the one G2 point of the search = 192), wire-format field elements.
BLSMI_API int blsmi_debug_hash_tail(int kind, const uint8_t* pts, uint8_t* out, uint8_t* good, size_t n) {
    if (kind < 0 || kind > 2 || (n && (!pts || !out || !good))) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    if (n > 4096) return BLSMI_E_ARG;
    const size_t rec = kind == 1 ? 384 : 192, hb = kind == 0 ? 96 : 192;
    const size_t prog = kind == 0 ? LAT_HASHFIN1_OFFSET : kind == 1 ? LAT_HASHFIN2_OFFSET : LAT_COFAC2_OFFSET;
    DBuf dp, dout, dg;
    HIPCHK(dp.alloc(rec * n)); HIPCHK(dout.alloc(hb * n)); HIPCHK(dg.alloc(n));
    HIPCHK(hipMemcpyAsync(dp.p, pts, rec * n, hipMemcpyHostToDevice, g_stream));
    launch_lat(prog, g_stream, {.b0 = {dp.p, rec}, .ok = dg.p, .out = dout.p}, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, hb * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(good, dg.p, n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// One launch of a unit program of the latency path (gen_lat.py: UNIT_PROGRAMS, appended to the image after the shipped programs): raw
// device-representation elements in, the limbs as the kernel left them (or a verdict byte) out.  n tuples of nin elements, one wave each.
BLSMI_API int blsmi_debug_lat_unit(int which, const int32_t* in_raw, size_t nin, size_t n, int32_t* out_raw, uint8_t* ok) {
    static const struct { size_t offset, nin, nout; } units[LAT_UNIT_COUNT] = LAT_UNIT_TABLE;      // nout 0: a verdict program (check1 / iszero)
    if (which < 0 || which >= LAT_UNIT_COUNT || nin != units[which].nin || n == 0 || n > 4096 || !in_raw) return BLSMI_E_ARG;
    const size_t prog = units[which].offset, nout = units[which].nout;
    if (nout ? !out_raw : !ok) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    DBuf din, dout, dok;
    HIPCHK(din.alloc(n * nin * 60)); HIPCHK(dout.alloc(std::max<size_t>(nout, 1) * 60 * n)); HIPCHK(dok.alloc(n));
    HIPCHK(hipMemcpyAsync(din.p, in_raw, n * nin * 60, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemsetAsync(dok.p, 0, n, g_stream));
    launch_lat(prog, g_stream, {.b3 = {din.p, nin * 60}, .ok = dok.p, .out = dout.p}, n);
    HIPCHK(hipGetLastError());
    if (nout) { HIPCHK(hipMemcpyAsync(out_raw, dout.p, nout * 60 * n, hipMemcpyDeviceToHost, g_stream)); }
    if (ok) { HIPCHK(hipMemcpyAsync(ok, dok.p, n, hipMemcpyDeviceToHost, g_stream)); }
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// the throughput tail of HashG1 (k_hash_g1_finish: sum of the two mapped points, 11-isogeny, cofactor clearing when clear != 0) on caller-chosen
// mapped points, and the flag a large aggregate's uncleared path raises when a message's two points cancel (*special bit 1; hash.cuh: swu_finish_g1)
BLSMI_API int blsmi_debug_hash_g1_finish(const uint8_t* pts, int clear, uint8_t* out, int* special, size_t n) {
    if (n && (!pts || !out || !special)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    DBuf dp, dout, dsp;
    HIPCHK(dp.alloc(192 * n)); HIPCHK(dout.alloc(96 * n)); HIPCHK(dsp.alloc(sizeof(int)));
    HIPCHK(hipMemcpyAsync(dp.p, pts, 192 * n, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemsetAsync(dsp.p, 0, sizeof(int), g_stream));
    if (clear == 2) {                                                       // the four-lanes-per-message tail and its redo pass (k_hash_quad.hip)
        DBuf dg; HIPCHK(dg.alloc(n));
        launch_quiet(KERNEL_OF(k_hash_g1_finish_quad), tuple_blocks(Layout::quad, n), g_stream, dp.p, dg.p, dout.p, n);
        launch_quiet(KERNEL_OF(k_hash_g1_finish_redo), nblocks(n), g_stream, dp.p, dg.p, dout.p, n);
        HIPCHK(hipGetLastError());
        std::vector<u8> hg(n);
        HIPCHK(hipMemcpyAsync(hg.data(), dg.p, n, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipMemcpyAsync(out, dout.p, 96 * n, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        *special = (int)std::count(hg.begin(), hg.end(), (u8)0);             // clear == 2: how many messages the quad kernel handed to the redo pass
        return BLSMI_OK;
    }
    launch_quiet(KERNEL_OF(k_hash_g1_finish), nblocks(n), g_stream, dp.p, dout.p, n, clear, dsp.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, 96 * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(special, dsp.p, sizeof(int), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// the kernel that re-hashes the messages whose good byte is 0 (out: in/out, records of the others are left alone)
BLSMI_API int blsmi_debug_hash_redo(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* good, uint8_t* out, size_t n) {
    if (kind < 0 || kind > 2 || (n && (!msgs || !off_or_domain || !good || !out))) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    const size_t hb = kind == 0 ? 96 : 192;
    DevMsgs dm(kind, off_or_domain, n); DBuf dout, dg;
    HIPCHK(dout.alloc(hb * n)); HIPCHK(dg.alloc(n));
    { int rc = dm.upload(msgs, off_or_domain, g_stream); if (rc) return rc; }
    HIPCHK(hipMemcpyAsync(dout.p, out, hb * n, hipMemcpyHostToDevice, g_stream));
    HIPCHK(hipMemcpyAsync(dg.p, good, n, hipMemcpyHostToDevice, g_stream));
    const unsigned g = nblocks(n);
    if (kind == 0) launch_quiet(KERNEL_OF(k_hash_g1_redo), g, g_stream, dm.m.p, dm.off.p, dg.p, dout.p, n);
    else if (kind == 1) launch_quiet(KERNEL_OF(k_hash_g2_redo), g, g_stream, dm.m.p, dm.off.p, dg.p, dout.p, n);
    else launch_quiet(KERNEL_OF(k_hash_g2_domain_redo), g, g_stream, dm.m.p, dm.off.p, dg.p, dout.p, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dout.p, hb * n, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}

BLSMI_API int blsmi_hash_g1_batch(const uint8_t* msgs, const uint64_t* off, uint8_t* out, size_t n) {
    return hash_host(0, msgs, off, out, n);
}
BLSMI_API int blsmi_hash_g2_batch(const uint8_t* msgs, const uint64_t* off, uint8_t* out, size_t n) {
    return hash_host(1, msgs, off, out, n);
}
BLSMI_API int blsmi_hash_g2_with_domain_batch(const uint8_t* msgs32, const uint8_t domain[8], uint8_t* out, size_t n) {
    return hash_host(2, msgs32, domain, out, n);
}

// Sign for n (message, secret key) pairs in one call: sig_i = sk_i * H(m_i) (g2pubs/bls.go:132-135, g1pubs/bls.go:132-135, 138-141) -- the hash
// points never leave the device between the two steps.  kind: 0 g2pubs (HashG1, 96-byte signatures), 1 g1pubs (HashG2, 192), 2 g1pubs
// WithDomain (HashG2WithDomain of 32-byte messages).  sks: n x 32 bytes big-endian.  out_inf[i] = 1 when the signature is the point at
// infinity (sk_i = 0 mod r: the reference returns the zero point).
int sign_host(int kind, const uint8_t* msgs, const void* off_or_domain, size_t off_bytes, size_t msg_bytes, const uint8_t* sks, uint8_t* out, uint8_t* out_inf, size_t n, uint64_t* out_jac = nullptr) {
    // out_jac (replaces out / out_inf): the signatures as in-memory Jacobian records, z = 1 ((0, 1, 0) for sk = 0 mod r)
    if (n && (!msgs || !off_or_domain || !sks || (out_jac ? false : (!out || !out_inf)))) return BLSMI_E_ARG;
    if (n == 0) return BLSMI_OK;
    { std::lock_guard<std::mutex> lk(g_mu); int rc = ensure_init_default(); if (rc) return rc; }
    const bool domain = kind == 2;
    const uint64_t* off = domain ? nullptr : static_cast<const uint64_t*>(off_or_domain);
    return run_shards(plan_shards(n, 64), [&](int, size_t lo, size_t hi) -> int {
        const GroupKernels& g = kind_of(kind).sig();
        const size_t m = hi - lo, OB = g.wire_bytes;
        const size_t mb = domain ? 32 * m : (size_t)(off[hi] - off[lo]);
        DBuf dm, doff, dh, dk, dout, dinf;
        HIPCHK(dm.alloc(mb)); HIPCHK(doff.alloc(domain ? 8 : sizeof(uint64_t) * (m + 1))); HIPCHK(dh.alloc(OB * m));
        HIPCHK(dk.alloc(32 * m)); HIPCHK(dout.alloc(OB * m)); HIPCHK(dinf.alloc(m));
        if (mb) HIPCHK(hipMemcpyAsync(dm.p, msgs + (domain ? 32 * lo : (size_t)off[lo]), mb, hipMemcpyHostToDevice, g_stream));
        if (domain) HIPCHK(hipMemcpyAsync(doff.p, off_or_domain, 8, hipMemcpyHostToDevice, g_stream));
        else if (lo == 0) HIPCHK(hipMemcpyAsync(doff.p, off, sizeof(uint64_t) * (m + 1), hipMemcpyHostToDevice, g_stream));
        else {                                                             // a later shard: offsets relative to its own first message
            std::vector<uint64_t> rel(m + 1);
            for (size_t i = 0; i <= m; i++) rel[i] = off[lo + i] - off[lo];
            HIPCHK(hipMemcpyAsync(doff.p, rel.data(), sizeof(uint64_t) * (m + 1), hipMemcpyHostToDevice, g_stream));
            HIPCHK(hipStreamSynchronize(g_stream));                        // (rel goes out of scope)
        }
        int rc = hash_dev(kind, dm.p, doff.p, dh.as<u8>(), m, g_stream, hash_route_alone(kind, m));
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(dk.p, sks + 32 * lo, 32 * m, hipMemcpyHostToDevice, g_stream));   // the keys travel while the hash runs
        rc = mul_dev_core(g, dh.as<u8>(), dk.as<u8>(), dout.as<u8>(), dinf.as<u8>(), m, g_stream);
        if (rc) return rc;
        if (out_jac) {
            const size_t jb = rec_bytes(OB, true);
            DBuf dj; HIPCHK(dj.alloc(jb * m));
            launch_quiet(KERNEL_OF(k_affine_to_jac), nblocks(m), g_stream, dout.p, dinf.p, 1, g.id, dj.p, m);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(reinterpret_cast<uint8_t*>(out_jac) + jb * lo, dj.p, jb * m, hipMemcpyDeviceToHost, g_stream));
            HIPCHK(hipStreamSynchronize(g_stream));
            return BLSMI_OK;
        }
        HIPCHK(hipMemcpyAsync(out + OB * lo, dout.p, OB * m, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipMemcpyAsync(out_inf + lo, dinf.p, m, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        return BLSMI_OK;
    });
}
BLSMI_API int blsmi_g2pubs_sign_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* sks, uint8_t* out_sigs, uint8_t* out_inf, size_t n) {
    return sign_host(0, msgs, off, sizeof(uint64_t) * (n + 1), (n && off) ? (size_t)off[n] : 0, sks, out_sigs, out_inf, n);
}
BLSMI_API int blsmi_g1pubs_sign_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* sks, uint8_t* out_sigs, uint8_t* out_inf, size_t n) {
    return sign_host(1, msgs, off, sizeof(uint64_t) * (n + 1), (n && off) ? (size_t)off[n] : 0, sks, out_sigs, out_inf, n);
}
BLSMI_API int blsmi_g1pubs_sign_with_domain_batch(const uint8_t* msgs32, const uint8_t domain[8], const uint8_t* sks, uint8_t* out_sigs, uint8_t* out_inf, size_t n) {
    return sign_host(2, msgs32, domain, 8, 32 * n, sks, out_sigs, out_inf, n);
}

// ... with the signatures handed back as the Go types hold them (Signature{s *bls.G?Projective}, z = 1)
BLSMI_API int blsmi_g2pubs_sign_batch_jac(const uint8_t* msgs, const uint64_t* off, const uint8_t* sks, uint64_t* out_sigs_jac, size_t n) {
    return sign_host(0, msgs, off, sizeof(uint64_t) * (n + 1), (n && off) ? (size_t)off[n] : 0, sks, nullptr, nullptr, n, out_sigs_jac);
}
BLSMI_API int blsmi_g1pubs_sign_batch_jac(const uint8_t* msgs, const uint64_t* off, const uint8_t* sks, uint64_t* out_sigs_jac, size_t n) {
    return sign_host(1, msgs, off, sizeof(uint64_t) * (n + 1), (n && off) ? (size_t)off[n] : 0, sks, nullptr, nullptr, n, out_sigs_jac);
}
BLSMI_API int blsmi_g1pubs_sign_with_domain_batch_jac(const uint8_t* msgs32, const uint8_t domain[8], const uint8_t* sks, uint64_t* out_sigs_jac, size_t n) {
    return sign_host(2, msgs32, domain, 8, 32 * n, sks, nullptr, nullptr, n, out_sigs_jac);
}
BLSMI_API int blsmi_g2pubs_verify_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags, uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    return verify_batch_host(0, msgs, off, pks, sigs, inf_flags, ok, ok_bitmap, n);
}
BLSMI_API int blsmi_g1pubs_verify_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags, uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    return verify_batch_host(1, msgs, off, pks, sigs, inf_flags, ok, ok_bitmap, n);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch(const uint8_t* msgs32, const uint8_t domain[8], const uint8_t* pks, const uint8_t* sigs, const uint8_t* inf_flags, uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    if (!domain) return BLSMI_E_ARG;
    return verify_batch_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), pks, sigs, inf_flags, ok, ok_bitmap, n);
}
BLSMI_API int blsmi_g2pubs_verify_batch_dev(const void* d_msgs, const void* d_off, const void* d_pks, const void* d_sigs, const void* d_inf, void* d_ok, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_msgs || !d_off || !d_pks || !d_sigs || !d_ok) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    return verify_batch_dev(0, d_msgs, d_off, d_pks, d_sigs, d_inf, d_ok, n, g_stream);
}
BLSMI_API int blsmi_g1pubs_verify_batch_dev(const void* d_msgs, const void* d_off, const void* d_pks, const void* d_sigs, const void* d_inf, void* d_ok, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_msgs || !d_off || !d_pks || !d_sigs || !d_ok) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    return verify_batch_dev(1, d_msgs, d_off, d_pks, d_sigs, d_inf, d_ok, n, g_stream);
}
// VerifyWithDomain (g1pubs/bls.go:171-174) over resident inputs: 32-byte messages, the 8-byte domain on the device as well
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_dev(const void* d_msgs32, const void* d_domain, const void* d_pks, const void* d_sigs, const void* d_inf, void* d_ok, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_msgs32 || !d_domain || !d_pks || !d_sigs || !d_ok) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    return verify_batch_dev(2, d_msgs32, d_domain, d_pks, d_sigs, d_inf, d_ok, n, g_stream);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t sig[96], size_t n, int* ok) {
    return verify_aggregate_host(0, msgs, off, pks, sig, n, ok, true);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t sig[192], size_t n, int* ok) {
    return verify_aggregate_host(1, msgs, off, pks, sig, n, ok, true);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_with_domain(const uint8_t* msgs32, const uint8_t domain[8], const uint8_t* pks, const uint8_t sig[192], size_t n, int* ok) {
    if (!domain) return BLSMI_E_ARG;
    return verify_aggregate_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), pks, sig, n, ok, false);   // no duplicate check (g1pubs/bls.go:300-311)
}
template <int KIND>
static int verify_aggregate_dev_api(const void* d_msgs, const void* d_off_or_domain, const void* d_pks, const uint8_t* sig, size_t n, int* ok, void* stream) {
    if (!ok || !sig || (n && (!d_msgs || !d_off_or_domain || !d_pks))) return BLSMI_E_ARG;
    *ok = 0;
    if (n == 0) {                                                          // nothing resident to locate a device by: any context serves
        LOCK_AND_INIT();
        UseStream us(stream);
        return verify_aggregate_dev(KIND, d_msgs, d_off_or_domain, d_pks, sig, 0, ok, KIND != 2);
    }
    LOCK_AND_INIT_AT(d_pks);
    UseStream us(stream);
    return verify_aggregate_dev(KIND, d_msgs, d_off_or_domain, d_pks, sig, n, ok, KIND != 2);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_dev(const void* d_msgs, const void* d_off, const void* d_pks, const uint8_t sig[96], size_t n, int* ok, void* stream) {
    return verify_aggregate_dev_api<0>(d_msgs, d_off, d_pks, sig, n, ok, stream);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_dev(const void* d_msgs, const void* d_off, const void* d_pks, const uint8_t sig[192], size_t n, int* ok, void* stream) {
    return verify_aggregate_dev_api<1>(d_msgs, d_off, d_pks, sig, n, ok, stream);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_with_domain_dev(const void* d_msgs32, const void* d_domain, const void* d_pks, const uint8_t sig[192], size_t n, int* ok, void* stream) {
    return verify_aggregate_dev_api<2>(d_msgs32, d_domain, d_pks, sig, n, ok, stream);
}
// ---- prepared public keys (k_prepared_pair.hip): G2AffineToPrepared once, Miller loops that read the lines ----------------
BLSMI_API int blsmi_g2_prepare_batch_dev(const void* d_g2_aff, size_t n, void* d_prepared, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_g2_aff || !d_prepared) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_prepared);
    UseStream us(stream);
    launch(KERNEL_OF(k_g2_prepare_pair), tuple_blocks(Layout::pair, n), g_stream, d_g2_aff, d_prepared, n);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
BLSMI_API int blsmi_g2_prepared_export_dev(const void* d_prepared, size_t n, void* d_out, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_prepared || !d_out) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    launch_quiet(KERNEL_OF(k_prepared_export), nblocks(408 * n), g_stream, d_prepared, d_out, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// G2AffineToPrepared of n host points, in the reference's own representation (the BenchmarkG2Prepare shape, pairing_test.go:60-81)
BLSMI_API int blsmi_g2_prepare_batch(const uint8_t* g2_aff, size_t n, uint64_t* out_coeffs) {
    if (n && (!g2_aff || !out_coeffs)) return BLSMI_E_ARG;
    LOCK_AND_INIT();
    if (n == 0) return BLSMI_OK;
    const size_t chunk_max = 32768;                                        // 0.8 GB of tables per pass
    for (size_t lo = 0; lo < n; lo += chunk_max) {
        const size_t m = std::min(chunk_max, n - lo);
        DBuf q, tab, o;
        HIPCHK(q.alloc(192 * m)); HIPCHK(tab.alloc(sizeof(i32) * blsmi_prep::WORDS * m)); HIPCHK(o.alloc(sizeof(u64) * 68 * 3 * 12 * m));
        HIPCHK(hipMemcpyAsync(q.p, g2_aff + 192 * lo, 192 * m, hipMemcpyHostToDevice, g_stream));
        launch(KERNEL_OF(k_g2_prepare_pair), tuple_blocks(Layout::pair, m), g_stream, q.p, tab.p, m);
        prof_mark(nullptr);
        launch_quiet(KERNEL_OF(k_prepared_export), nblocks(408 * m), g_stream, tab.p, o.p, m);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out_coeffs + (size_t)68 * 3 * 12 * lo, o.p, sizeof(u64) * 68 * 3 * 12 * m, hipMemcpyDeviceToHost, g_stream));
        HIPCHK(hipStreamSynchronize(g_stream));
        tl_ctx->arena.reset();
    }
    return BLSMI_OK;
}
// For callers without a HIP runtime of their own (the cgo shim): the library allocates the tables on the calling thread's device
// (device 0 unless blsmi_init chose another), prepares n host keys into them and hands back the device pointer as the handle.
// jac: the keys are in-memory Jacobian records (blsmi 0.6), brought to affine on the device (upload_points)
static int g2_prepared_create(const uint8_t* g2, bool jac, size_t n, void** handle) {
    if (!handle || !n || !g2) return BLSMI_E_ARG;
    *handle = nullptr;
    LOCK_AND_INIT();
    void* tab = nullptr;
    HIPCHK(hipMalloc(&tab, (size_t)BLSMI_G2_PREPARED_BYTES * n));
    auto code = [](hipError_t e) { return e == hipSuccess ? BLSMI_OK : e == hipErrorOutOfMemory ? BLSMI_E_NOMEM : BLSMI_E_HIP; };
    DBuf q;
    int rc = code(q.alloc(192 * n));
    if (!rc) rc = jac ? upload_points(group_kernels(2), true, g2, q.p, n, g_stream) : code(hipMemcpyAsync(q.p, g2, 192 * n, hipMemcpyHostToDevice, g_stream));
    if (!rc) {
        launch(KERNEL_OF(k_g2_prepare_pair), tuple_blocks(Layout::pair, n), g_stream, q.p, tab, n);
        prof_mark(nullptr);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g_stream);
        rc = (jac && e != hipSuccess) ? BLSMI_E_HIP : code(e);             // (the in-memory form reports every failure of the kernel as HIP)
    }
    if (rc) { (void)hipStreamSynchronize(g_stream); (void)hipFree(tab); return rc; }   // (nothing queued may still write the tables)
    *handle = tab;
    return BLSMI_OK;
}
BLSMI_API int blsmi_g2_prepared_create(const uint8_t* g2_aff, size_t n, void** handle) { return g2_prepared_create(g2_aff, false, n, handle); }
BLSMI_API int blsmi_g2_prepared_destroy(void* handle) {
    if (!handle) return BLSMI_OK;
    const int idx = device_index_of_pointer(handle);
    if (idx < 0) return BLSMI_E_ARG;
    CtxLease lease(idx);                                                   // makes the owning device current; waits for a free context of it
    if (lease.rc) return lease.rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipFree(handle));
    return BLSMI_OK;
}
// n g2pubs.Verify()s, messages and signatures in host memory, the keys prepared (tables on one device: the call runs there, unsplit)
BLSMI_API int blsmi_g2pubs_verify_batch_prepared(const uint8_t* msgs, const uint64_t* off, const void* d_prepared, const uint32_t* key_idx, const uint8_t* sigs,
                                                 const uint8_t* inf_flags, uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    if (n == 0) return BLSMI_OK;
    if (!msgs || !off || !d_prepared || !sigs || (!ok && !ok_bitmap)) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_prepared);
    return verify_batch_leased(0, msgs, off, nullptr, sigs, inf_flags, ok, ok_bitmap, n, nullptr, (const i32*)d_prepared, key_idx);
}
BLSMI_API int blsmi_pairing_batch_prepared_dev(const void* d_g1, const void* d_prepared, const void* d_key_idx, void* d_out, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_g1 || !d_prepared || !d_out) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    const PrepKeys prep{(const i32*)d_prepared, (const u32*)d_key_idx};
    const Layout lay = pairing_layout(0, n, tune(), route_load(n));
    if (!prepared_tables_serve(Call::pairing, lay, tune())) {              // the layouts without table-reading kernels run on the keys' affine records
        DBuf pk; int rc = prep_gather_keys(prep, pk, n, g_stream); if (rc) return rc;
        return pairing_dev(d_g1, pk.p, d_out, n, g_stream, 0, lay);
    }
    HIPCHK(g_ws.reserve(sizeof(i32) * 12 * NL * n));
    i32* f = reinterpret_cast<i32*>(g_ws.p);
    const unsigned pblocks = (unsigned)((n + PT - 1) / PT);
    launch(KERNEL_OF(k_miller1_prep_pair), pblocks, g_stream, d_g1, prep.tables, prep.idx, f, n);
    launch(KERNEL_OF(k_final_exp_pair), pblocks, g_stream, f, d_out, n, 0);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
BLSMI_API int blsmi_g2pubs_verify_batch_prepared_dev(const void* d_msgs, const void* d_off, const void* d_prepared, const void* d_key_idx, const void* d_sigs, const void* d_inf, void* d_ok, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_msgs || !d_off || !d_prepared || !d_sigs || !d_ok) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    const PrepKeys prep{(const i32*)d_prepared, (const u32*)d_key_idx};
    return verify_batch_dev(0, d_msgs, d_off, nullptr, d_sigs, d_inf, d_ok, n, g_stream, &prep);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_prepared_dev(const void* d_msgs, const void* d_off, const void* d_prepared, const void* d_key_idx, const uint8_t sig[96], size_t n, int* ok, void* stream) {
    if (!ok || !sig || (n && (!d_msgs || !d_off || !d_prepared))) return BLSMI_E_ARG;
    *ok = 0;
    if (n == 0) { LOCK_AND_INIT(); UseStream us(stream); return verify_aggregate_dev(0, d_msgs, d_off, nullptr, sig, 0, ok, true); }
    LOCK_AND_INIT_AT(d_prepared);
    UseStream us(stream);
    const PrepKeys prep{(const i32*)d_prepared, (const u32*)d_key_idx};
    return verify_aggregate_dev(0, d_msgs, d_off, nullptr, sig, n, ok, true, &prep);
}
// Signature.VerifyAggregate with messages, key indices and the signature in HOST memory and the keys prepared (the cgo shim's form)
// fmt: FMT_SIG_JAC -- the signature is an in-memory Jacobian record
static int verify_aggregate_prepared_host(const uint8_t* msgs, const uint64_t* off, const void* d_prepared, const uint32_t* key_idx, const uint8_t* sig, size_t n, int* ok, int fmt) {
    if (!ok || !sig || (n && (!msgs || !off || !d_prepared))) return BLSMI_E_ARG;
    *ok = 0;
    if (n == 0) return verify_aggregate_host(0, msgs, off, nullptr, sig, 0, ok, true, fmt);
    LOCK_AND_INIT_AT(d_prepared);
    DevMsgs dm(0, off, n); DBuf didx;
    HIPCHK(didx.alloc(sizeof(uint32_t) * n));
    { int rc = dm.upload(msgs, off, g_stream); if (rc) return rc; }
    if (key_idx) HIPCHK(hipMemcpyAsync(didx.p, key_idx, sizeof(uint32_t) * n, hipMemcpyHostToDevice, g_stream));
    const PrepKeys prep{(const i32*)d_prepared, key_idx ? didx.as<u32>() : nullptr};
    return verify_aggregate_dev(0, dm.m.p, dm.off.p, nullptr, sig, n, ok, true, &prep, fmt);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_prepared(const uint8_t* msgs, const uint64_t* off, const void* d_prepared, const uint32_t* key_idx, const uint8_t sig[96], size_t n, int* ok) {
    return verify_aggregate_prepared_host(msgs, off, d_prepared, key_idx, sig, n, ok, 0);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_common(const uint8_t* msg, size_t msg_len, const uint8_t* pks, const uint8_t sig[96], size_t n, int* ok) {
    return verify_aggregate_common_host(0, msg, msg_len, nullptr, pks, sig, n, ok);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common(const uint8_t* msg, size_t msg_len, const uint8_t* pks, const uint8_t sig[192], size_t n, int* ok) {
    return verify_aggregate_common_host(1, msg, msg_len, nullptr, pks, sig, n, ok);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain(const uint8_t msg32[32], const uint8_t domain[8], const uint8_t* pks, const uint8_t sig[192], size_t n, int* ok) {
    if (!domain) return BLSMI_E_ARG;
    return verify_aggregate_common_host(2, msg32, 32, domain, pks, sig, n, ok);
}
// device-pointer forms of VerifyAggregateCommon (g2pubs/bls.go:275-278, g1pubs/bls.go:287-297): the n keys resident in HBM
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_dev(const void* d_pks, size_t n, const uint8_t* msg, size_t msg_len, const uint8_t sig[96], int* ok, void* stream) {
    if (!ok || !sig || (msg_len && !msg) || (n && !d_pks)) return BLSMI_E_ARG;
    if (n == 0) return verify_aggregate_common_host(0, msg ? msg : (const uint8_t*)"", msg_len, nullptr, nullptr, sig, 0, ok);
    LOCK_AND_INIT_AT(d_pks);
    UseStream us(stream);
    return verify_aggregate_common_dev(0, d_pks, n, msg, msg_len, nullptr, sig, ok);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_dev(const void* d_pks, size_t n, const uint8_t* msg, size_t msg_len, const uint8_t sig[192], int* ok, void* stream) {
    if (!ok || !sig || (msg_len && !msg) || (n && !d_pks)) return BLSMI_E_ARG;
    if (n == 0) return verify_aggregate_common_host(1, msg ? msg : (const uint8_t*)"", msg_len, nullptr, nullptr, sig, 0, ok);
    LOCK_AND_INIT_AT(d_pks);
    UseStream us(stream);
    return verify_aggregate_common_dev(1, d_pks, n, msg, msg_len, nullptr, sig, ok);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_dev(const void* d_pks, size_t n, const uint8_t msg32[32], const uint8_t domain[8], const uint8_t sig[192], int* ok, void* stream) {
    if (!ok || !sig || !msg32 || !domain || (n && !d_pks)) return BLSMI_E_ARG;
    if (n == 0) return verify_aggregate_common_host(2, msg32, 32, domain, nullptr, sig, 0, ok);
    LOCK_AND_INIT_AT(d_pks);
    UseStream us(stream);
    return verify_aggregate_common_dev(2, d_pks, n, msg32, 32, domain, sig, ok);
}
BLSMI_API int blsmi_g2pubs_verify_serialized_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, int check_subgroup, uint8_t* ok, uint8_t* err_pk, uint8_t* err_sig, size_t n) {
    return verify_serialized_host(0, msgs, off, pks, sigs, check_subgroup, ok, err_pk, err_sig, n);
}
BLSMI_API int blsmi_g1pubs_verify_serialized_batch(const uint8_t* msgs, const uint64_t* off, const uint8_t* pks, const uint8_t* sigs, int check_subgroup, uint8_t* ok, uint8_t* err_pk, uint8_t* err_sig, size_t n) {
    return verify_serialized_host(1, msgs, off, pks, sigs, check_subgroup, ok, err_pk, err_sig, n);
}
BLSMI_API int blsmi_g1_decompress_batch(const uint8_t* in, int check, uint8_t* out, uint8_t* out_inf, uint8_t* err, size_t n) { return decompress_host(1, in, check, out, out_inf, err, n); }
BLSMI_API int blsmi_g2_decompress_batch(const uint8_t* in, int check, uint8_t* out, uint8_t* out_inf, uint8_t* err, size_t n) { return decompress_host(2, in, check, out, out_inf, err, n); }
BLSMI_API int blsmi_g1_compress_batch(const uint8_t* pts, const uint8_t* in_inf, uint8_t* out, size_t n) { return compress_host(1, pts, in_inf, out, n); }
BLSMI_API int blsmi_g2_compress_batch(const uint8_t* pts, const uint8_t* in_inf, uint8_t* out, size_t n) { return compress_host(2, pts, in_inf, out, n); }
BLSMI_API int blsmi_g1_check_batch(const uint8_t* pts, const uint8_t* in_inf, int check, uint8_t* status, size_t n) { return check_host(1, false, pts, in_inf, check, status, n); }
BLSMI_API int blsmi_g2_check_batch(const uint8_t* pts, const uint8_t* in_inf, int check, uint8_t* status, size_t n) { return check_host(2, false, pts, in_inf, check, status, n); }
BLSMI_API int blsmi_g1_check_batch_jac(const uint64_t* pts_jac, int check, uint8_t* status, size_t n) { return check_host(1, true, reinterpret_cast<const uint8_t*>(pts_jac), nullptr, check, status, n); }
BLSMI_API int blsmi_g2_check_batch_jac(const uint64_t* pts_jac, int check, uint8_t* status, size_t n) { return check_host(2, true, reinterpret_cast<const uint8_t*>(pts_jac), nullptr, check, status, n); }
BLSMI_API int blsmi_g1_check_batch_dev(const void* d_pts, const void* d_in_inf, int jac, int check, void* d_status, size_t n, void* stream) { return check_dev_api(1, d_pts, d_in_inf, jac, check, d_status, n, stream); }
BLSMI_API int blsmi_g2_check_batch_dev(const void* d_pts, const void* d_in_inf, int jac, int check, void* d_status, size_t n, void* stream) { return check_dev_api(2, d_pts, d_in_inf, jac, check, d_status, n, stream); }
BLSMI_API int blsmi_g1_decompress_batch_jac(const uint8_t* in, int check, uint64_t* out_jac, uint8_t* out_inf, uint8_t* err, size_t n) { return decompress_jac_host(1, in, check, out_jac, out_inf, err, n); }
BLSMI_API int blsmi_g2_decompress_batch_jac(const uint8_t* in, int check, uint64_t* out_jac, uint8_t* out_inf, uint8_t* err, size_t n) { return decompress_jac_host(2, in, check, out_jac, out_inf, err, n); }
BLSMI_API int blsmi_g1_compress_batch_jac(const uint64_t* pts_jac, uint8_t* out, size_t n) { return compress_jac_host(1, pts_jac, out, n); }
BLSMI_API int blsmi_g2_compress_batch_jac(const uint64_t* pts_jac, uint8_t* out, size_t n) { return compress_jac_host(2, pts_jac, out, n); }
BLSMI_API int blsmi_g1_decompress_batch_jac_dev(const void* d_in, int check, void* d_out_jac, void* d_out_inf, void* d_err, size_t n, void* stream) { return decompress_jac_dev_api(1, d_in, check, d_out_jac, d_out_inf, d_err, n, stream); }
BLSMI_API int blsmi_g2_decompress_batch_jac_dev(const void* d_in, int check, void* d_out_jac, void* d_out_inf, void* d_err, size_t n, void* stream) { return decompress_jac_dev_api(2, d_in, check, d_out_jac, d_out_inf, d_err, n, stream); }
BLSMI_API int blsmi_g1_compress_batch_jac_dev(const void* d_pts_jac, void* d_out, size_t n, void* stream) { return compress_jac_dev_api(1, d_pts_jac, d_out, n, stream); }
BLSMI_API int blsmi_g2_compress_batch_jac_dev(const void* d_pts_jac, void* d_out, size_t n, void* stream) { return compress_jac_dev_api(2, d_pts_jac, d_out, n, stream); }

// ---- the verify surface over the reference's in-memory points (blsmi 0.6; include/blsmi.h "in-memory points") ---------------------------
// Keys and signatures as the Go values hold them: bls.G2Projective = 36 x u64, bls.G1Projective = 18 x u64 (x, y, z; FQ = 6 LE u64 Montgomery
// limbs).  z == 0 is the point at infinity (verdict 0 where the reference panics), so there are no infinity flags to pass.
#define JACP(p) reinterpret_cast<const uint8_t*>(p)
BLSMI_API int blsmi_g2pubs_verify_batch_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    return verify_batch_host(0, msgs, off, JACP(pks), JACP(sigs), nullptr, ok, ok_bitmap, n, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_batch_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    return verify_batch_host(1, msgs, off, JACP(pks), JACP(sigs), nullptr, ok, ok_bitmap, n, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_jac(const uint8_t* msgs32, const uint8_t domain[8], const uint64_t* pks, const uint64_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    if (!domain) return BLSMI_E_ARG;
    return verify_batch_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), JACP(pks), JACP(sigs), nullptr, ok, ok_bitmap, n, FMT_JAC);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t sig[18], size_t n, int* ok) {
    return verify_aggregate_host(0, msgs, off, JACP(pks), JACP(sig), n, ok, true, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_jac(const uint8_t* msgs, const uint64_t* off, const uint64_t* pks, const uint64_t sig[36], size_t n, int* ok) {
    return verify_aggregate_host(1, msgs, off, JACP(pks), JACP(sig), n, ok, true, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_with_domain_jac(const uint8_t* msgs32, const uint8_t domain[8], const uint64_t* pks, const uint64_t sig[36], size_t n, int* ok) {
    if (!domain) return BLSMI_E_ARG;
    return verify_aggregate_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), JACP(pks), JACP(sig), n, ok, false, FMT_JAC);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_jac(const uint8_t* msg, size_t msg_len, const uint64_t* pks, const uint64_t sig[18], size_t n, int* ok) {
    return verify_aggregate_common_host(0, msg, msg_len, nullptr, JACP(pks), JACP(sig), n, ok, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_jac(const uint8_t* msg, size_t msg_len, const uint64_t* pks, const uint64_t sig[36], size_t n, int* ok) {
    return verify_aggregate_common_host(1, msg, msg_len, nullptr, JACP(pks), JACP(sig), n, ok, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_jac(const uint8_t msg32[32], const uint8_t domain[8], const uint64_t* pks, const uint64_t sig[36], size_t n, int* ok) {
    if (!domain) return BLSMI_E_ARG;
    return verify_aggregate_common_host(2, msg32, 32, domain, JACP(pks), JACP(sig), n, ok, FMT_JAC);
}
// device-pointer forms: messages, offsets (kind 2: the 8-byte domain) and the in-memory points resident on one of the library's devices
template <int KIND>
static int verify_batch_jac_dev_api(const void* d_msgs, const void* d_off, const void* d_pks, const void* d_sigs, void* d_ok, size_t n, void* stream) {
    if (n == 0) return BLSMI_OK;
    if (!d_msgs || !d_off || !d_pks || !d_sigs || !d_ok) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    const Kind k = kind_of(KIND);
    DBuf p, sg;
    HIPCHK(p.alloc((size_t)k.pk_bytes * n)); HIPCHK(sg.alloc((size_t)k.sig_bytes * n));
    int rc = jac_to_wire_dev(k.pk(), d_pks, p.p, nullptr, n, g_stream);
    if (!rc) rc = jac_to_wire_dev(k.sig(), d_sigs, sg.p, nullptr, n, g_stream);
    if (rc) return rc;
    return verify_batch_dev(KIND, d_msgs, d_off, p.p, sg.p, nullptr, d_ok, n, g_stream);
}
BLSMI_API int blsmi_g2pubs_verify_batch_jac_dev(const void* d_msgs, const void* d_off, const void* d_pks, const void* d_sigs, void* d_ok, size_t n, void* stream) {
    return verify_batch_jac_dev_api<0>(d_msgs, d_off, d_pks, d_sigs, d_ok, n, stream);
}
BLSMI_API int blsmi_g1pubs_verify_batch_jac_dev(const void* d_msgs, const void* d_off, const void* d_pks, const void* d_sigs, void* d_ok, size_t n, void* stream) {
    return verify_batch_jac_dev_api<1>(d_msgs, d_off, d_pks, d_sigs, d_ok, n, stream);
}
BLSMI_API int blsmi_g1pubs_verify_with_domain_batch_jac_dev(const void* d_msgs32, const void* d_domain, const void* d_pks, const void* d_sigs, void* d_ok, size_t n, void* stream) {
    return verify_batch_jac_dev_api<2>(d_msgs32, d_domain, d_pks, d_sigs, d_ok, n, stream);
}
// prepared keys (g2pubs) from, and verified against, in-memory points
BLSMI_API int blsmi_g2_prepared_create_jac(const uint64_t* g2_jac, size_t n, void** handle) { return g2_prepared_create(JACP(g2_jac), true, n, handle); }
BLSMI_API int blsmi_g2pubs_verify_batch_prepared_jac(const uint8_t* msgs, const uint64_t* off, const void* d_prepared, const uint32_t* key_idx, const uint64_t* sigs,
                                                     uint8_t* ok, uint8_t* ok_bitmap, size_t n) {
    if (n == 0) return BLSMI_OK;
    if (!msgs || !off || !d_prepared || !sigs || (!ok && !ok_bitmap)) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_prepared);
    return verify_batch_leased(0, msgs, off, nullptr, JACP(sigs), nullptr, ok, ok_bitmap, n, nullptr, (const i32*)d_prepared, key_idx, FMT_SIG_JAC);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_prepared_jac(const uint8_t* msgs, const uint64_t* off, const void* d_prepared, const uint32_t* key_idx, const uint64_t sig[18], size_t n, int* ok) {
    return verify_aggregate_prepared_host(msgs, off, d_prepared, key_idx, JACP(sig), n, ok, FMT_SIG_JAC);
}
#undef JACP

// ---- segmented sums and batches of VerifyAggregateCommon (blsmi 0.9; include/blsmi.h "committees") ------------------------------------
// m sums over ragged, index-addressed subsets of one key table: segment j is {pts[idx[k]] : seg_off[j] <= k < seg_off[j + 1]} (idx null:
// the positions themselves).  The chunk plan is built here from seg_off (k_curve.hip: segsum_chunk_body): pass 1 cuts every segment into
// chunks of at most K positions, a lane (G2 affine: a lane pair) per chunk; each fold pass cuts every segment's partials into chunks of at
// most max(K, 2) until no segment has more than 64; the final kernel adds those across one wave per segment.
// K: the "segsum_chunk" option, 0 = from the total count T.  Eight positions per lane while that still leaves 2^16 chunks (below, the
// passes are latency-bound: the chain of 8 + 8 + ... dependent additions is what a call waits for), then doubled up to 64.
namespace {
size_t segsum_auto_chunk(size_t total) {
    size_t K = 8;
    while (total / K > ((size_t)1 << 16) && K < 64) K *= 2;
    return K;
}
struct SegPlan {
    size_t m = 0, K = 0, nch1 = 0;
    struct Fold { size_t nsrc, nch, lo, cnt; };                            // lo / cnt: byte offsets of the pass's chunk arrays in `blob`
    std::vector<Fold> folds;
    size_t ch_lo = 0, ch_cnt = 0, ch_seg = 0, seg_lo = 0, seg_cnt = 0, nlast = 0;
    std::vector<uint8_t> blob;                                             // every array of the plan, uploaded in one copy
    template <class T> size_t put(const std::vector<T>& v) {
        const size_t at = (blob.size() + 7) & ~(size_t)7;
        blob.resize(at + sizeof(T) * v.size());
        if (!v.empty()) memcpy(blob.data() + at, v.data(), sizeof(T) * v.size());
        return at;
    }
};
// the host forms' checks (BLSMI_E_ARG before any device work): offsets from 0, non-decreasing; every index below npk
int segsum_check(size_t npk, const uint32_t* idx, const uint64_t* seg_off, size_t m) {
    if (!seg_off || seg_off[0] != 0) return BLSMI_E_ARG;
    for (size_t j = 0; j < m; j++) if (seg_off[j + 1] < seg_off[j]) return BLSMI_E_ARG;
    const uint64_t total = seg_off[m];
    if (!idx) return total <= npk ? BLSMI_OK : BLSMI_E_ARG;
    for (uint64_t k = 0; k < total; k++) if (idx[k] >= npk) return BLSMI_E_ARG;
    return BLSMI_OK;
}
// last_max: the partials a segment may still have when the final pass takes over (the sums: one wave adds up to 64 across its lanes)
// K1: the chunk size of pass 1 alone (0: K, as the folds; the weighted sums take 1 -- one 64-bit ladder per lane, segsum_dev)
void segsum_plan(const uint64_t* seg_off, size_t m, size_t K, SegPlan& p, size_t last_max = 64, size_t K1 = 0) {
    p.m = m; p.K = K;
    if (K1 == 0) K1 = K;
    std::vector<uint64_t> lo, part_lo(m);
    std::vector<uint32_t> cnt, seg, part_cnt(m);
    for (size_t j = 0; j < m; j++) {
        const uint64_t a = seg_off[j], len = seg_off[j + 1] - a;
        part_lo[j] = lo.size();
        for (uint64_t c = 0; c < len; c += K1) { lo.push_back(a + c); cnt.push_back((uint32_t)std::min<uint64_t>(K1, len - c)); seg.push_back((uint32_t)j); }
        part_cnt[j] = (uint32_t)(lo.size() - part_lo[j]);
    }
    p.nch1 = lo.size();
    p.ch_lo = p.put(lo); p.ch_cnt = p.put(cnt); p.ch_seg = p.put(seg);
    size_t nsrc = p.nch1;
    const size_t Kf = std::max<size_t>(K, 2);
    while (m && *std::max_element(part_cnt.begin(), part_cnt.end()) > last_max) {
        lo.clear(); cnt.clear();
        for (size_t j = 0; j < m; j++) {
            const uint64_t a = part_lo[j], len = part_cnt[j];
            part_lo[j] = lo.size();
            for (uint64_t c = 0; c < len; c += Kf) { lo.push_back(a + c); cnt.push_back((uint32_t)std::min<uint64_t>(Kf, len - c)); }
            part_cnt[j] = (uint32_t)(lo.size() - part_lo[j]);
        }
        p.folds.push_back({nsrc, lo.size(), p.put(lo), p.put(cnt)});
        nsrc = lo.size();
    }
    p.nlast = nsrc;
    p.seg_lo = p.put(part_lo); p.seg_cnt = p.put(part_cnt);
}
// The segmented sum on the device, everything on stream s, not synchronised (the temporaries come from the call's arena, `p.blob` is read
// by the copy: both stay alive until the caller synchronises).  jac: d_pts are in-memory Jacobian records (no d_in_inf).
// d_out: m affine records, d_out_inf: m bytes (1 infinity, bad_code for a segment with an index >= npk, 0 otherwise).
// d_scalars (may be null; affine points only): npk 64-bit weights -- segment j is then sum scalars[i] * pts[i] over its indices i, pass 1
// running the ladder (k_g?_segsum_chunk_u64) over a plan whose first pass has chunks of one position.  u64_pass1 (may be null: the
// one-lane kernel, as the forms of 0.11 to 0.13 and blsmi_g?_sum_segmented_u64 run it): the row's entry that runs the weighted pass 1
// instead -- g.segsum_chunk_u64_opt, G2's lane-pair ladder unless the options say one lane.
int segsum_dev(const GroupKernels& g, bool jac, const void* d_pts, const u8* d_in_inf, size_t npk, const u32* d_idx, const SegPlan& p, u8* d_out, u8* d_out_inf,
               u8 bad_code, hipStream_t s, const u64* d_scalars = nullptr, const SegsumU64Pass1* u64_pass1 = nullptr) {
    const size_t m = p.m;
    if (m == 0) return BLSMI_OK;
    const size_t words = (size_t)g.fq * NL + 1;
    DBuf plan, bad, a, b;
    HIPCHK(plan.alloc(p.blob.size())); HIPCHK(bad.alloc(m));
    HIPCHK(hipMemcpyAsync(plan.p, p.blob.data(), p.blob.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(bad.p, 0, m, s));
    auto at64 = [&](size_t off) { return reinterpret_cast<const u64*>(plan.as<u8>() + off); };
    auto at32 = [&](size_t off) { return reinterpret_cast<const u32*>(plan.as<u8>() + off); };
    HIPCHK(a.alloc(sizeof(i32) * words * p.nch1));
    const size_t n1 = p.nch1;
    if (n1 && d_scalars) {
        if (jac) return BLSMI_E_ARG;
        const bool mark = tl_ctx && s == tl_ctx->stream;                   // (profile marks are events on the context's main stream)
        const SegsumU64Pass1 pass1 = u64_pass1 ? *u64_pass1 : SegsumU64Pass1{g.segsum_chunk_u64, Layout::single};
        if (mark) prof_mark(pass1.k.name);
        launch_items_quiet(pass1, n1, s, d_pts, d_in_inf, npk, d_scalars, d_idx, at64(p.ch_lo), at32(p.ch_cnt), at32(p.ch_seg), bad.p, a.p, n1);
        if (mark) prof_mark(nullptr);
    } else if (n1) {
        if (jac) launch_quiet(g.segsum_chunk_jac, nblocks(n1), s, d_pts, npk, d_idx, at64(p.ch_lo), at32(p.ch_cnt), at32(p.ch_seg), bad.p, a.p, n1);
        else launch_items_quiet(g.segsum_chunk, n1, s, d_pts, d_in_inf, npk, d_idx, at64(p.ch_lo), at32(p.ch_cnt), at32(p.ch_seg), bad.p, a.p, n1);
    }
    i32* src = a.as<i32>();
    for (const SegPlan::Fold& f : p.folds) {
        DBuf d; HIPCHK(d.alloc(sizeof(i32) * words * f.nch));
        launch_items_quiet(g.segsum_fold, f.nch, s, src, f.nsrc, at64(f.lo), at32(f.cnt), d.p, f.nch);
        src = d.as<i32>();
    }
    launch_quiet(g.segsum_final, m, s, src, p.nlast, at64(p.seg_lo), at32(p.seg_cnt), bad.p, bad_code, d_out, d_out_inf);
    HIPCHK(hipGetLastError());
    return BLSMI_OK;
}
size_t segsum_chunk_of(size_t total) { const size_t K = tune().segsum_chunk; return K ? K : segsum_auto_chunk(total); }
// host forms: everything checked here first, then one lease
// weighted (not with jac): the _u64 forms, scalars are npk 64-bit weights
int sum_segmented_host(int group, bool jac, const uint8_t* pts, const uint8_t* in_inf, size_t npk, const uint32_t* idx, const uint64_t* seg_off, size_t m,
                       uint8_t* out, uint8_t* out_inf, bool weighted = false, const uint64_t* scalars = nullptr, const SegsumU64Pass1* u64_pass1 = nullptr) {
    if (m == 0) return BLSMI_OK;
    if (!out || !out_inf || (npk && !pts) || (weighted && npk && !scalars)) return BLSMI_E_ARG;
    int rc = segsum_check(npk, idx, seg_off, m);
    if (rc) return rc;
    LOCK_AND_INIT();
    const GroupKernels& g = group_kernels(group);
    const size_t pb = g.wire_bytes, pin = rec_bytes(pb, jac), total = seg_off[m];
    SegPlan plan;
    segsum_plan(seg_off, m, segsum_chunk_of(total), plan, 64, weighted ? 1 : 0);
    DBuf dp, di, dx, dout, dinf, dsc;
    if (weighted) { HIPCHK(dsc.alloc(sizeof(uint64_t) * npk)); if (npk) HIPCHK(hipMemcpyAsync(dsc.p, scalars, sizeof(uint64_t) * npk, hipMemcpyHostToDevice, g_stream)); }
    HIPCHK(dp.alloc(pin * npk)); HIPCHK(di.alloc(npk)); HIPCHK(dx.alloc(sizeof(uint32_t) * total)); HIPCHK(dout.alloc(pb * m)); HIPCHK(dinf.alloc(m));
    if (npk) HIPCHK(hipMemcpyAsync(dp.p, pts, pin * npk, hipMemcpyHostToDevice, g_stream));
    if (in_inf && !jac && npk) HIPCHK(hipMemcpyAsync(di.p, in_inf, npk, hipMemcpyHostToDevice, g_stream));
    if (idx && total) HIPCHK(hipMemcpyAsync(dx.p, idx, sizeof(uint32_t) * total, hipMemcpyHostToDevice, g_stream));
    rc = segsum_dev(g, jac, dp.p, (in_inf && !jac) ? di.as<u8>() : nullptr, npk, idx ? dx.as<u32>() : nullptr, plan, dout.as<u8>(), dinf.as<u8>(), 2, g_stream,
                    weighted ? dsc.as<u64>() : nullptr, u64_pass1);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, dout.p, pb * m, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipMemcpyAsync(out_inf, dinf.p, m, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
// the m + 1 offsets of a _dev call, fetched to the host (those calls synchronise anyway) and checked: from 0, non-decreasing
int segsum_fetch_offsets(const void* d_seg_off, size_t m, std::vector<uint64_t>& off) {
    off.resize(m + 1);
    HIPCHK(hipMemcpyAsync(off.data(), d_seg_off, sizeof(uint64_t) * (m + 1), hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    if (off[0] != 0) return BLSMI_E_ARG;
    for (size_t j = 0; j < m; j++) if (off[j + 1] < off[j]) return BLSMI_E_ARG;
    return BLSMI_OK;
}
int sum_segmented_dev_api(int group, const void* d_pts, const void* d_in_inf, size_t npk, const void* d_idx, const void* d_seg_off, size_t m,
                          void* d_out, void* d_out_inf, void* stream) {
    if (m == 0) return BLSMI_OK;
    if (!d_seg_off || !d_out || !d_out_inf || (npk && !d_pts)) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_out);
    UseStream us(stream);
    std::vector<uint64_t> off;
    int rc = segsum_fetch_offsets(d_seg_off, m, off);
    if (rc) return rc;
    SegPlan plan;
    segsum_plan(off.data(), m, segsum_chunk_of(off[m]), plan);
    rc = segsum_dev(group_kernels(group), false, d_pts, (const u8*)d_in_inf, npk, (const u32*)d_idx, plan, (u8*)d_out, (u8*)d_out_inf, 2, g_stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
}  // namespace
BLSMI_API int blsmi_g1_sum_segmented(const uint8_t* pts, const uint8_t* in_inf, size_t npk, const uint32_t* idx, const uint64_t* seg_off, size_t m, uint8_t* out, uint8_t* out_inf) {
    return sum_segmented_host(1, false, pts, in_inf, npk, idx, seg_off, m, out, out_inf);
}
BLSMI_API int blsmi_g2_sum_segmented(const uint8_t* pts, const uint8_t* in_inf, size_t npk, const uint32_t* idx, const uint64_t* seg_off, size_t m, uint8_t* out, uint8_t* out_inf) {
    return sum_segmented_host(2, false, pts, in_inf, npk, idx, seg_off, m, out, out_inf);
}
BLSMI_API int blsmi_g1_sum_segmented_u64(const uint8_t* pts, const uint8_t* in_inf, size_t npk, const uint64_t* scalars, const uint32_t* idx, const uint64_t* seg_off, size_t m, uint8_t* out, uint8_t* out_inf) {
    return sum_segmented_host(1, false, pts, in_inf, npk, idx, seg_off, m, out, out_inf, true, scalars);
}
BLSMI_API int blsmi_g2_sum_segmented_u64(const uint8_t* pts, const uint8_t* in_inf, size_t npk, const uint64_t* scalars, const uint32_t* idx, const uint64_t* seg_off, size_t m, uint8_t* out, uint8_t* out_inf) {
    return sum_segmented_host(2, false, pts, in_inf, npk, idx, seg_off, m, out, out_inf, true, scalars);
}
// blsmi_g2_sum_segmented_u64 with pass 1 through the lane-pair ladder (k_g2_segsum_chunk_u64_pair) whatever the options say: the parity test's way to it
BLSMI_API int blsmi_debug_g2_sum_segmented_u64_pair(const uint8_t* pts, const uint8_t* in_inf, size_t npk, const uint64_t* scalars, const uint32_t* idx, const uint64_t* seg_off, size_t m, uint8_t* out, uint8_t* out_inf) {
    return sum_segmented_host(2, false, pts, in_inf, npk, idx, seg_off, m, out, out_inf, true, scalars, &group_kernels(2, true).segsum_chunk_u64_opt);
}
BLSMI_API int blsmi_g1_sum_segmented_jac(const uint64_t* pts_jac, size_t npk, const uint32_t* idx, const uint64_t* seg_off, size_t m, uint8_t* out, uint8_t* out_inf) {
    return sum_segmented_host(1, true, reinterpret_cast<const uint8_t*>(pts_jac), nullptr, npk, idx, seg_off, m, out, out_inf);
}
BLSMI_API int blsmi_g2_sum_segmented_jac(const uint64_t* pts_jac, size_t npk, const uint32_t* idx, const uint64_t* seg_off, size_t m, uint8_t* out, uint8_t* out_inf) {
    return sum_segmented_host(2, true, reinterpret_cast<const uint8_t*>(pts_jac), nullptr, npk, idx, seg_off, m, out, out_inf);
}
BLSMI_API int blsmi_g1_sum_segmented_dev(const void* d_pts, const void* d_in_inf, size_t npk, const void* d_idx, const void* d_seg_off, size_t m, void* d_out, void* d_out_inf, void* stream) {
    return sum_segmented_dev_api(1, d_pts, d_in_inf, npk, d_idx, d_seg_off, m, d_out, d_out_inf, stream);
}
BLSMI_API int blsmi_g2_sum_segmented_dev(const void* d_pts, const void* d_in_inf, size_t npk, const void* d_idx, const void* d_seg_off, size_t m, void* d_out, void* d_out_inf, void* stream) {
    return sum_segmented_dev_api(2, d_pts, d_in_inf, npk, d_idx, d_seg_off, m, d_out, d_out_inf, stream);
}

// Item j of a batch: VerifyAggregateCommon(sig_j, committee j, msg_j) -- the committee's sum (the segmented sum above, on aux[1], while the
// m messages are hashed), its flags (infinity, empty, bad index) as bit 0 of the tuple flags, then the m Verify()s of verify_batch_dev,
// routed by m as any batch of m tuples.  One lease, one device.  The caller holds the lease; every buffer is on its device.
namespace {
int agg_common_batch_dev(int kind, const void* d_msgs, const void* d_off_or_domain, const void* d_pks, size_t npk, const u32* d_idx, const SegPlan& plan,
                         const void* d_sigs, void* d_ok, bool pks_jac) {
    const Kind k = kind_of(kind);
    const size_t m = plan.m;
    DBuf dagg, dinf;
    HIPCHK(dagg.alloc((size_t)k.pk_bytes * m)); HIPCHK(dinf.alloc(m));
    HIPCHK(tl_ctx->ensure_aux());
    hipStream_t side = tl_ctx->aux[1];
    HIPCHK(hipEventRecord(tl_ctx->fork, g_stream)); HIPCHK(hipStreamWaitEvent(side, tl_ctx->fork, 0));   // (the keys and indices may still be arriving on g_stream)
    int rc = segsum_dev(k.pk(), pks_jac, d_pks, nullptr, npk, d_idx, plan, dagg.as<u8>(), dinf.as<u8>(), 1, side);
    if (rc) return rc;
    HIPCHK(hipEventRecord(tl_ctx->join[1], side));
    return verify_batch_dev(kind, d_msgs, d_off_or_domain, dagg.p, d_sigs, dinf.p, d_ok, m, g_stream, nullptr, tl_ctx->join[1]);   // synchronises
}
int agg_common_batch_host(int kind, const uint8_t* msgs, const uint64_t* off_or_domain, const uint8_t* pks, size_t npk, const uint32_t* idx, const uint64_t* seg_off,
                          const uint8_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t m, int fmt = 0) {
    if (m == 0) return BLSMI_OK;
    if (!sigs || !off_or_domain || (!ok && !ok_bitmap) || (npk && !pks)) return BLSMI_E_ARG;
    if (kind != 2) {                                                       // message offsets: from 0, non-decreasing
        if (off_or_domain[0] != 0) return BLSMI_E_ARG;
        for (size_t j = 0; j < m; j++) if (off_or_domain[j + 1] < off_or_domain[j]) return BLSMI_E_ARG;
    }
    DevMsgs dm(kind, off_or_domain, m);
    if (dm.msg_bytes && !msgs) return BLSMI_E_ARG;
    int rc = segsum_check(npk, idx, seg_off, m);
    if (rc) return rc;
    const Kind k = kind_of(kind);
    const bool pj = (fmt & FMT_PK_JAC) != 0;
    const size_t pin = rec_bytes(k.pk_bytes, pj), total = seg_off[m];
    { std::lock_guard<std::mutex> lk(g_mu); int rc0 = ensure_init_default(); if (rc0) return rc0; }
    CtxLease lease;
    if (lease.rc) return lease.rc;
    SegPlan plan;
    segsum_plan(seg_off, m, segsum_chunk_of(total), plan);
    DBuf dp, dx, ds, dok;
    HIPCHK(dp.alloc(pin * npk)); HIPCHK(dx.alloc(sizeof(uint32_t) * total));
    HIPCHK(ds.alloc((size_t)k.sig_bytes * m)); HIPCHK(dok.alloc(m));
    if (npk) HIPCHK(hipMemcpyAsync(dp.p, pks, pin * npk, hipMemcpyHostToDevice, g_stream));
    if (idx && total) HIPCHK(hipMemcpyAsync(dx.p, idx, sizeof(uint32_t) * total, hipMemcpyHostToDevice, g_stream));
    rc = dm.upload(msgs, off_or_domain, g_stream);
    if (rc) return rc;
    rc = upload_points(k.sig(), (fmt & FMT_SIG_JAC) != 0, sigs, ds.p, m, g_stream);
    if (rc) return rc;
    rc = agg_common_batch_dev(kind, dm.m.p, dm.off.p, dp.p, npk, idx ? dx.as<u32>() : nullptr, plan, ds.p, dok.p, pj);
    if (rc) return rc;
    return fetch_verdicts(dok.p, ok, ok_bitmap, m, g_stream);
}
template <int KIND>
static int agg_common_batch_dev_api(const void* d_msgs, const void* d_off_or_domain, const void* d_pks, size_t npk, const void* d_idx, const void* d_seg_off,
                                    const void* d_sigs, void* d_ok, size_t m, void* stream) {
    if (m == 0) return BLSMI_OK;
    if (!d_msgs || !d_off_or_domain || !d_seg_off || !d_sigs || !d_ok || (npk && !d_pks)) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_ok);
    UseStream us(stream);
    std::vector<uint64_t> off;
    int rc = segsum_fetch_offsets(d_seg_off, m, off);
    if (rc) return rc;
    SegPlan plan;
    segsum_plan(off.data(), m, segsum_chunk_of(off[m]), plan);
    return agg_common_batch_dev(KIND, d_msgs, d_off_or_domain, d_pks, npk, (const u32*)d_idx, plan, d_sigs, d_ok, false);
}
}  // namespace
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_batch(const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pks, size_t npk, const uint32_t* idx, const uint64_t* seg_off,
                                                         const uint8_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t m) {
    return agg_common_batch_host(0, msgs, msg_off, pks, npk, idx, seg_off, sigs, ok, ok_bitmap, m);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_batch(const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* pks, size_t npk, const uint32_t* idx, const uint64_t* seg_off,
                                                         const uint8_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t m) {
    return agg_common_batch_host(1, msgs, msg_off, pks, npk, idx, seg_off, sigs, ok, ok_bitmap, m);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_batch(const uint8_t* msgs32, const uint8_t domain[8], const uint8_t* pks, size_t npk, const uint32_t* idx,
                                                                     const uint64_t* seg_off, const uint8_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t m) {
    return agg_common_batch_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), pks, npk, idx, seg_off, sigs, ok, ok_bitmap, m);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_batch_jac(const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* pks, size_t npk, const uint32_t* idx, const uint64_t* seg_off,
                                                             const uint64_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t m) {
    return agg_common_batch_host(0, msgs, msg_off, reinterpret_cast<const uint8_t*>(pks), npk, idx, seg_off, reinterpret_cast<const uint8_t*>(sigs), ok, ok_bitmap, m, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_batch_jac(const uint8_t* msgs, const uint64_t* msg_off, const uint64_t* pks, size_t npk, const uint32_t* idx, const uint64_t* seg_off,
                                                             const uint64_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t m) {
    return agg_common_batch_host(1, msgs, msg_off, reinterpret_cast<const uint8_t*>(pks), npk, idx, seg_off, reinterpret_cast<const uint8_t*>(sigs), ok, ok_bitmap, m, FMT_JAC);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_jac(const uint8_t* msgs32, const uint8_t domain[8], const uint64_t* pks, size_t npk, const uint32_t* idx,
                                                                         const uint64_t* seg_off, const uint64_t* sigs, uint8_t* ok, uint8_t* ok_bitmap, size_t m) {
    return agg_common_batch_host(2, msgs32, reinterpret_cast<const uint64_t*>(domain), reinterpret_cast<const uint8_t*>(pks), npk, idx, seg_off,
                                 reinterpret_cast<const uint8_t*>(sigs), ok, ok_bitmap, m, FMT_JAC);
}
BLSMI_API int blsmi_g2pubs_verify_aggregate_common_batch_dev(const void* d_msgs, const void* d_msg_off, const void* d_pks, size_t npk, const void* d_idx, const void* d_seg_off,
                                                             const void* d_sigs, void* d_ok, size_t m, void* stream) {
    return agg_common_batch_dev_api<0>(d_msgs, d_msg_off, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, stream);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_batch_dev(const void* d_msgs, const void* d_msg_off, const void* d_pks, size_t npk, const void* d_idx, const void* d_seg_off,
                                                             const void* d_sigs, void* d_ok, size_t m, void* stream) {
    return agg_common_batch_dev_api<1>(d_msgs, d_msg_off, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, stream);
}
BLSMI_API int blsmi_g1pubs_verify_aggregate_common_with_domain_batch_dev(const void* d_msgs32, const void* d_domain, const void* d_pks, size_t npk, const void* d_idx,
                                                                         const void* d_seg_off, const void* d_sigs, void* d_ok, size_t m, void* stream) {
    return agg_common_batch_dev_api<2>(d_msgs32, d_domain, d_pks, npk, d_idx, d_seg_off, d_sigs, d_ok, m, stream);
}

// ---- pairing products (blsmi 0.10; include/blsmi.h "pairing products") ------------------------------------------------------------------
// Item j = FinalExponentiation(MillerLoop({(P_k, Q_k) : seg_off[j] <= k < seg_off[j + 1]})) (pairing.go:16-75, 79-129) in three stages on the
// call's stream: one Miller value per pair in the layout a Pairing call of np tuples takes (any Miller value serves a product that is
// final-exponentiated, so the wave layout runs "miller1raw"); the segmented product of those values, a lane row per chunk (k_fq12_seg.hip)
// over the chunk plan of the segmented sums (segsum_plan; fold passes until a segment has at most max(K, 2) partials, K as the sums choose
// it); the final exponentiation of the m products in the layout blsmi_final_exponentiation_batch gives m values (beyond lat_max: a Pairing
// call's quad / pair kernels), then the comparison with one.  A pair with a point at infinity runs its loop on the generators and is left out of the product.  One lease, one device.
namespace {
// one Miller value per tuple into the hand-off buffer f, the tuples free of points at infinity
void launch_miller_tuples(const u8* d_g1, const u8* d_g2, i32* f, size_t n, hipStream_t s, Layout l) {
    if (l == Layout::wave) launch_lat_marked(LAT_MILLER1RAW_OFFSET, s, {.b0 = {d_g1, 96}, .b1 = {d_g2, 192}, .out = f}, n);
    else launch(kernels_of(l).miller1h, tuple_blocks(l, n), s, d_g1, d_g2, f, n);
}
void pprod_plan(const uint64_t* seg_off, size_t m, SegPlan& plan) {
    const size_t K = segsum_chunk_of(seg_off[m]);
    segsum_plan(seg_off, m, K, plan, std::max<size_t>(K, 2));
}
// the final exponentiation's layout for m values: what blsmi_final_exponentiation_batch gives them (wave, row), and beyond those -- where that
// entry point has only its one-lane kernel -- the quad / pair kernels a Pairing call of m tuples ends in
Layout pprod_fe_layout(size_t m, size_t load) {
    const Layout fe = final_exp_layout(m, tune(), load);
    return fe == Layout::single && tune().pair_layout ? (m <= tune().quad_max ? Layout::quad : Layout::pair) : fe;
}
// The segmented product of the nsrc values at src over `plan`, whose arrays are on the device at d_blob: pass 1 (skip: the values it leaves
// out, or null), the folds, the final pass.  Its m records go to dst (a hand-off buffer) and / or out_m384 (the reference's in-memory form).
int seg_prod_dev(const i32* src, size_t nsrc, const u8* skip, const SegPlan& plan, const u8* d_blob, i32* dst, u64* out_m384, hipStream_t s) {
    const size_t words = (size_t)12 * NL;
    auto at64 = [&](size_t off) { return reinterpret_cast<const u64*>(d_blob + off); };
    auto at32 = [&](size_t off) { return reinterpret_cast<const u32*>(d_blob + off); };
    if (plan.nch1) {
        DBuf d; HIPCHK(d.alloc(sizeof(i32) * words * plan.nch1));
        launch_quiet(KERNEL_OF(k_fq12_seg_prod_row), tuple_blocks(Layout::row, plan.nch1), s, src, nsrc, skip, at64(plan.ch_lo), at32(plan.ch_cnt), d.p, nullptr, plan.nch1);
        src = d.as<i32>(); nsrc = plan.nch1;
    }
    for (const SegPlan::Fold& fo : plan.folds) {
        DBuf d; HIPCHK(d.alloc(sizeof(i32) * words * fo.nch));
        launch_quiet(KERNEL_OF(k_fq12_seg_prod_row), tuple_blocks(Layout::row, fo.nch), s, src, nsrc, nullptr, at64(fo.lo), at32(fo.cnt), d.p, nullptr, fo.nch);
        src = d.as<i32>(); nsrc = fo.nch;
    }
    launch_quiet(KERNEL_OF(k_fq12_seg_prod_row), tuple_blocks(Layout::row, plan.m), s, src, nsrc, nullptr, at64(plan.seg_lo), at32(plan.seg_cnt), dst, out_m384, plan.m);
    return BLSMI_OK;
}
// The final exponentiation of m values in the layout fe -- prod: 576-byte in-memory records for the wave layout, a hand-off buffer otherwise --
// into `out` (576 bytes each) and, where d_is_one is given, their comparison with one.  Leaves the profile mark open.
void final_exp_values(Layout fe, const void* prod, u64* out, void* d_is_one, size_t m, hipStream_t s) {
    if (fe == Layout::wave) launch_lat_marked(LAT_FINALEXP1_OFFSET, s, {.b0 = {prod, 576}, .out = out}, m);
    else launch(kernels_of(fe).final_exp, tuple_blocks(fe, m), s, prod, out, m, 0);
    if (d_is_one) {
        launch(KERNEL_OF(k_fq12_is_one_m384), tuple_blocks(Layout::row, m), s, out, d_is_one, m);
    }
}
// d_g1 / d_g2: np affine records the call owns (records of skipped pairs are overwritten); d_flags: np flag bytes or null.  The m values go to
// d_out (576 bytes each) and / or the m verdict bytes to d_is_one.  Synchronises.
int pprod_dev(u8* d_g1, u8* d_g2, const u8* d_flags, size_t np, const SegPlan& plan, void* d_out, void* d_is_one, hipStream_t s) {
    const size_t m = plan.m, words = (size_t)12 * NL;
    DBuf skip, f, blob, prod, vals;
    HIPCHK(blob.alloc(plan.blob.size()));
    HIPCHK(hipMemcpyAsync(blob.p, plan.blob.data(), plan.blob.size(), hipMemcpyHostToDevice, s));
    const Layout fe = pprod_fe_layout(m, route_load(np));
    const i32* src = nullptr;
    if (np) {
        HIPCHK(skip.alloc(np)); HIPCHK(f.alloc(sizeof(i32) * words * np));
        launch_quiet(KERNEL_OF(k_pprod_skip), nblocks(np), s, d_g1, d_g2, d_flags, g_gens.g1, g_gens.g2, skip.p, np);
        launch_miller_tuples(d_g1, d_g2, f.as<i32>(), np, s, pairing_layout(0, np, tune(), route_load(np)));
        src = f.as<i32>();
    }
    // the product (its records: the final exponentiation's input -- the reference's in-memory form for the wave layout, the hand-off buffer otherwise)
    prof_mark(KERNEL_OF(k_fq12_seg_prod_row).name);                         // one segment: the passes of seg_prod_dev
    HIPCHK(prod.alloc(fe == Layout::wave ? 576 * m : sizeof(i32) * words * m));
    int rc = seg_prod_dev(src, np, skip.as<u8>(), plan, blob.as<u8>(), fe == Layout::wave ? (i32*)nullptr : prod.as<i32>(), fe == Layout::wave ? prod.as<u64>() : (u64*)nullptr, s);
    if (rc) return rc;
    u64* out = (u64*)d_out;
    if (!out) { HIPCHK(vals.alloc(576 * m)); out = vals.as<u64>(); }
    final_exp_values(fe, prod.p, out, d_is_one, m, s);
    prof_mark(nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    return BLSMI_OK;
}
// the offsets of a product: from 0, non-decreasing, ending at np (pprod_rlc_plan.h has the rule; a null pointer fails it)
int pprod_check(const uint64_t* seg_off, size_t m, size_t np) {
    return blsmi_route::pprod_rlc_offsets_valid(seg_off, m, np) ? BLSMI_OK : BLSMI_E_ARG;
}
int pprod_host(const uint8_t* g1, const uint8_t* g2, const uint8_t* inf_flags, size_t np, const uint64_t* seg_off, size_t m, uint64_t* out_fq12, uint8_t* is_one, bool jac) {
    if (m == 0) return BLSMI_OK;
    if ((!out_fq12 && !is_one) || (np && (!g1 || !g2))) return BLSMI_E_ARG;
    int rc = pprod_check(seg_off, m, np);
    if (rc) return rc;
    LOCK_AND_INIT();
    SegPlan plan;
    pprod_plan(seg_off, m, plan);
    DBuf a, b, fl, o, ok;
    HIPCHK(a.alloc(96 * np)); HIPCHK(b.alloc(192 * np)); HIPCHK(fl.alloc(np)); HIPCHK(o.alloc(576 * m)); HIPCHK(ok.alloc(m));
    if (np) {
        rc = upload_points(group_kernels(1), jac, g1, a.p, np, g_stream);
        if (!rc) rc = upload_points(group_kernels(2), jac, g2, b.p, np, g_stream);
        if (rc) return rc;
        if (inf_flags) HIPCHK(hipMemcpyAsync(fl.p, inf_flags, np, hipMemcpyHostToDevice, g_stream));
    }
    rc = pprod_dev(a.as<u8>(), b.as<u8>(), inf_flags ? fl.as<u8>() : nullptr, np, plan, out_fq12 ? o.p : nullptr, is_one ? ok.p : nullptr, g_stream);
    if (rc) return rc;
    if (out_fq12) HIPCHK(hipMemcpyAsync(out_fq12, o.p, 576 * m, hipMemcpyDeviceToHost, g_stream));
    if (is_one) HIPCHK(hipMemcpyAsync(is_one, ok.p, m, hipMemcpyDeviceToHost, g_stream));
    HIPCHK(hipStreamSynchronize(g_stream));
    return BLSMI_OK;
}
int pprod_dev_api(const void* d_g1, const void* d_g2, const void* d_inf_flags, size_t np, const void* d_seg_off, size_t m, void* d_out_fq12, void* d_is_one, void* stream, bool jac) {
    if (m == 0) return BLSMI_OK;
    if (!d_seg_off || (!d_out_fq12 && !d_is_one) || (np && (!d_g1 || !d_g2))) return BLSMI_E_ARG;
    LOCK_AND_INIT_AT(d_out_fq12 ? d_out_fq12 : d_is_one);
    UseStream us(stream);
    std::vector<uint64_t> off;
    int rc = segsum_fetch_offsets(d_seg_off, m, off);
    if (rc) return rc;
    if (off[m] != np) return BLSMI_E_ARG;
    SegPlan plan;
    pprod_plan(off.data(), m, plan);
    DBuf a, b;                                                             // the call's own copies: the records of skipped pairs are overwritten
    HIPCHK(a.alloc(96 * np)); HIPCHK(b.alloc(192 * np));
    if (np && jac) {
        rc = jac_to_wire_dev(group_kernels(1), d_g1, a.p, nullptr, np, g_stream);
        if (!rc) rc = jac_to_wire_dev(group_kernels(2), d_g2, b.p, nullptr, np, g_stream);
        if (rc) return rc;
    } else if (np) {
        HIPCHK(hipMemcpyAsync(a.p, d_g1, 96 * np, hipMemcpyDeviceToDevice, g_stream));
        HIPCHK(hipMemcpyAsync(b.p, d_g2, 192 * np, hipMemcpyDeviceToDevice, g_stream));
    }
    return pprod_dev(a.as<u8>(), b.as<u8>(), (const u8*)d_inf_flags, np, plan, d_out_fq12, d_is_one, g_stream);
}
}  // namespace
BLSMI_API int blsmi_pairing_product_batch(const uint8_t* g1_aff, const uint8_t* g2_aff, const uint8_t* inf_flags, size_t np, const uint64_t* seg_off, size_t m,
                                          uint64_t* out_fq12, uint8_t* is_one) {
    return pprod_host(g1_aff, g2_aff, inf_flags, np, seg_off, m, out_fq12, is_one, false);
}
BLSMI_API int blsmi_pairing_product_batch_jac(const uint64_t* g1_jac, const uint64_t* g2_jac, size_t np, const uint64_t* seg_off, size_t m, uint64_t* out_fq12, uint8_t* is_one) {
    return pprod_host(reinterpret_cast<const uint8_t*>(g1_jac), reinterpret_cast<const uint8_t*>(g2_jac), nullptr, np, seg_off, m, out_fq12, is_one, true);
}
BLSMI_API int blsmi_pairing_product_batch_dev(const void* d_g1_aff, const void* d_g2_aff, const void* d_inf_flags, size_t np, const void* d_seg_off, size_t m,
                                              void* d_out_fq12, void* d_is_one, void* stream) {
    return pprod_dev_api(d_g1_aff, d_g2_aff, d_inf_flags, np, d_seg_off, m, d_out_fq12, d_is_one, stream, false);
}
BLSMI_API int blsmi_pairing_product_batch_jac_dev(const void* d_g1_jac, const void* d_g2_jac, size_t np, const void* d_seg_off, size_t m, void* d_out_fq12, void* d_is_one, void* stream) {
    return pprod_dev_api(d_g1_jac, d_g2_jac, nullptr, np, d_seg_off, m, d_out_fq12, d_is_one, stream, true);
}
