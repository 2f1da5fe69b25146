// places_api.hip — the vo_vocab_* and vo_places_* entry points of libvo_hip.so: a vocabulary of visual words trained on the device, one
// histogram per keyframe, and the loop query over the histograms (include/vo_hip.h, "place recognition").  Host code only; the kernels
// are in reloc_kernels.hip, beside the nearest-neighbour bodies the quantiser calls.
#include "vo_host.h"

#define VO_VOCAB_MIN_K 256
#define VO_VOCAB_MAX_K 4096
#define VO_VOCAB_MAX_ROWS (1 << 22)           // 2 * 255 * rows + rows stays below 2^31: k_vocab_update's rounding in int32
#define VO_PLACES_MAX_ENTRIES 65536
#define VO_PLACES_MAX_TOP_K 16

static bool vocab_k_ok(int K) { return K >= VO_VOCAB_MIN_K && K <= VO_VOCAB_MAX_K && K % 256 == 0; }

// The vocabulary's rows and the buffers of training and quantising, for K words under the configuration as it stands.  Kept while
// the next vocabulary has the same shape; otherwise released as a whole and made again.  Either way the vocabulary is no longer
// valid and the index is closed: the caller is about to write new words.
static int vocab_reserve(vo_ctx* ctx, const Batch& b, int K)
{
    VocabState& V = ctx->vocab;
    const int D = b.sift ? 128 : 32;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->places = PlacesState();
    V.valid = false;
    if (V.b.v.rows && V.b.v.D == D && V.K == K && V.F_cap == b.max_frames && V.kp_cap == b.kp_cap) return VO_OK;
    if ((size_t)b.max_frames * b.kp_cap >= ((size_t)1 << 31)) FAIL(VO_ERR_INVALID, "max_frames x kp_cap must fit 32-bit indices");
    ctx->vocab = VocabState();
    const size_t k = (size_t)K, F = (size_t)b.max_frames, C = (size_t)b.kp_cap;
    DevList& mem = V.mem; VocabBuf& vb = V.b;
    HIPCHK(mem.alloc(&vb.v.rows, k * D)); HIPCHK(mem.alloc(&vb.v.flag, 1));
    if (b.sift) { HIPCHK(mem.alloc(&vb.v.img, k * 128)); HIPCHK(mem.alloc(&vb.v.norms, k)); }
    HIPCHK(mem.alloc(&vb.tmp, k * D)); HIPCHK(mem.alloc(&vb.acc, k * (b.sift ? 128 : 256))); HIPCHK(mem.alloc(&vb.cnt, k));
    HIPCHK(mem.alloc(&vb.slots, F)); HIPCHK(mem.alloc(&vb.word, F * C)); HIPCHK(mem.alloc(&vb.prev, F * C));
    HIPCHK(mem.alloc(&vb.changed, 1)); HIPCHK(mem.alloc(&vb.key, k)); HIPCHK(mem.alloc(&vb.ids, F));
    vb.v.D = D; vb.v.cap_rows = K; vb.v.npt = K; vb.v.xyz = nullptr;
    V.K = K; V.F_cap = b.max_frames; V.kp_cap = b.kp_cap;
    return VO_OK;
}

// F slots of a call: in range, at most max_frames of them; their keypoint counts (host copy) and, under SIFT, no slot flagged for its
// descriptor norm.  counts[q] = rows of slots[q].
static int places_slots_check(vo_ctx* ctx, const Batch& b, const int32_t* slots, int F, const char* who, std::vector<int>* counts)
{
    if (F < 0 || F > b.max_frames || (F > 0 && !slots)) FAIL(VO_ERR_INVALID, "%s: 0 <= F <= max_frames slots, got %d", who, F);
    for (int q = 0; q < F; q++) if (slots[q] < 0 || slots[q] >= b.max_frames) FAIL(VO_ERR_INVALID, "%s: slot %d out of range", who, (int)slots[q]);
    counts->assign((size_t)F, 0);
    if (F == 0) return VO_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<int> all((size_t)b.max_frames), fl;
    HIPCHK(hipMemcpy(all.data(), b.kp_count, all.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (b.sift) { fl.resize(all.size()); HIPCHK(hipMemcpy(fl.data(), b.flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost)); }
    for (int q = 0; q < F; q++) {
        (*counts)[q] = std::min(std::max(all[(size_t)slots[q]], 0), b.kp_cap);
        if (b.sift && (fl[(size_t)slots[q]] & 2)) FAIL(VO_ERR_INVALID, "%s: a SIFT descriptor row broke the norm bound of the integer matcher (slot %d)", who, (int)slots[q]);
    }
    return VO_OK;
}

// the words of F slots into vb.word (vb.slots uploaded here); the caller waits for the stream before `slots` goes away
static int quantise(vo_ctx* ctx, const Batch& b, const int32_t* slots, int F)
{
    const VocabBuf& vb = ctx->vocab.b;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(vb.slots, slots, (size_t)F * sizeof(int), hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_MATCH_NN); launch_vocab_assign(s, vb, F, b.desc, b.desc_x, b.norms, b.kp_count, b.kp_cap, desc_x_rows(b.kp_cap)); }
    HIPCHK(hipGetLastError());
    return VO_OK;
}

extern "C" int vo_vocab_train(vo_ctx* ctx, const int32_t* slots, int F, int K, int iterations, int32_t* iterations_run)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_vocab_train: vo_batch_configure[_sift] has not been called");
    if (!vocab_k_ok(K)) FAIL(VO_ERR_INVALID, "vo_vocab_train: K must be a multiple of 256 in 256 .. 4096, got %d", K);
    if (F < 1) FAIL(VO_ERR_INVALID, "vo_vocab_train: at least one slot is needed");
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int> cnt;
    int rc = places_slots_check(ctx, b, slots, F, "vo_vocab_train", &cnt); if (rc) return rc;
    long long n = 0;
    for (int q = 0; q < F; q++) n += cnt[q];
    if (n < K) FAIL(VO_ERR_TOO_FEW, "vo_vocab_train: %lld descriptor rows cannot start %d words", n, K);
    if (n > VO_VOCAB_MAX_ROWS) FAIL(VO_ERR_UNSUPPORTED, "vo_vocab_train: at most %d training rows, got %lld", VO_VOCAB_MAX_ROWS, n);
    rc = vocab_reserve(ctx, b, K); if (rc) return rc;
    VocabState& V = ctx->vocab;
    const VocabBuf& vb = V.b;
    hipStream_t s = ctx->stream;
    // word w starts as training row floor(w n / K)
    std::vector<int> key((size_t)K);
    {
        int q = 0; long long first = 0;                     // slot q holds training rows first .. first + cnt[q] - 1
        for (int w = 0; w < K; w++) {
            const long long r = (long long)w * n / K;
            while (r >= first + cnt[q]) { first += cnt[q]; q++; }
            key[w] = slots[q] * b.kp_cap + (int)(r - first);
        }
    }
    const size_t acc_n = (size_t)K * (b.sift ? 128 : 256);
    HIPCHK(hipMemcpyAsync(vb.key, key.data(), (size_t)K * sizeof(int), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(vb.v.flag, 0, sizeof(int), s));
    HIPCHK(hipMemsetAsync(vb.prev, 0xff, (size_t)F * b.kp_cap * sizeof(int), s));
    { StageTimer t(ctx, ST_MISC); launch_vocab_store(s, vb, b.desc, vb.key); }
    HIPCHK(hipGetLastError());
    const int rounds = iterations < 1 ? 1 : iterations;
    int done = 0;
    for (int r = 0; r < rounds; r++) {
        rc = quantise(ctx, b, slots, F); if (rc) return rc;
        {
            StageTimer t(ctx, ST_MISC);
            HIPCHK(hipMemsetAsync(vb.acc, 0, acc_n * sizeof(int), s)); HIPCHK(hipMemsetAsync(vb.cnt, 0, (size_t)K * sizeof(int), s));
            HIPCHK(hipMemsetAsync(vb.changed, 0, sizeof(int), s));
            launch_vocab_accumulate(s, vb, F, b.desc, b.kp_count, b.kp_cap);
        }
        HIPCHK(hipGetLastError());
        int changed = 0;
        HIPCHK(hipMemcpyAsync(&changed, vb.changed, sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));                    // the one read of a round
        if (ctx->prof) prof_collect(ctx);
        if (r > 0 && changed == 0) break;                   // the update would write the words it read
        { StageTimer t(ctx, ST_MISC); launch_vocab_update(s, vb); }
        HIPCHK(hipGetLastError());
        done++;
    }
    int flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, vb.v.flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    if (flag & 2) FAIL(VO_ERR_INVALID, "vo_vocab_train: a SIFT word broke the norm bound of the integer matcher (|row|^2 > 2^20)");
    V.valid = true;
    if (iterations_run) *iterations_run = done;
    return VO_OK;
}

extern "C" int vo_vocab_set(vo_ctx* ctx, const uint8_t* words, int K)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_vocab_set: vo_batch_configure[_sift] has not been called");
    if (!vocab_k_ok(K)) FAIL(VO_ERR_INVALID, "vo_vocab_set: K must be a multiple of 256 in 256 .. 4096, got %d", K);
    if (!words) FAIL(VO_ERR_INVALID, "vo_vocab_set: words are needed");
    const size_t D = b.sift ? 128 : 32;
    if (b.sift)                                             // checked here, so that a refused vocabulary changes nothing
        for (int w = 0; w < K; w++) {
            long long sq = 0;
            for (size_t j = 0; j < D; j++) sq += (long long)words[(size_t)w * D + j] * words[(size_t)w * D + j];
            if (sq > (1 << 20)) FAIL(VO_ERR_INVALID, "vo_vocab_set: SIFT word %d breaks the norm bound of the integer matcher (|row|^2 > 2^20)", w);
        }
    HIPCHK(hipSetDevice(ctx->device));
    int rc = vocab_reserve(ctx, b, K); if (rc) return rc;
    rc = ctx->staging.grow(ctx, (size_t)K * D); if (rc) return rc;
    VocabState& V = ctx->vocab;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(ctx->staging.p, words, (size_t)K * D, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(V.b.v.flag, 0, sizeof(int), s));
    { StageTimer t(ctx, ST_MISC); launch_vocab_store(s, V.b, ctx->staging.p, nullptr); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    V.valid = true;
    return VO_OK;
}

extern "C" int vo_vocab_get(vo_ctx* ctx, uint8_t* words, int cap, int32_t* K)
{
    if (!ctx) return VO_ERR_INVALID;
    const VocabState& V = ctx->vocab;
    if (!V.valid) FAIL(VO_ERR_INVALID, "vo_vocab_get: there is no vocabulary (vo_vocab_train, vo_vocab_set)");
    if (!K || cap < 0) FAIL(VO_ERR_INVALID, "bad arguments");
    *K = V.K;
    const size_t n = (size_t)std::min(cap, V.K);
    if (n == 0 || !words) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(words, V.b.v.rows, n * V.b.v.D, hipMemcpyDeviceToHost));
    return VO_OK;
}

extern "C" int vo_vocab_words(vo_ctx* ctx, int slot, int32_t* word, int cap, int32_t* n_out)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_vocab_words: vo_batch_configure[_sift] has not been called");
    if (!ctx->vocab.valid) FAIL(VO_ERR_INVALID, "vo_vocab_words: there is no vocabulary (vo_vocab_train, vo_vocab_set)");
    if (!n_out || cap < 0) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    const int32_t sl = slot;
    std::vector<int> cnt;
    int rc = places_slots_check(ctx, b, &sl, 1, "vo_vocab_words", &cnt); if (rc) return rc;
    rc = quantise(ctx, b, &sl, 1); if (rc) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->prof) prof_collect(ctx);
    *n_out = cnt[0];
    const size_t n = (size_t)std::min(cap, cnt[0]);
    if (n > 0 && word) HIPCHK(hipMemcpy(word, ctx->vocab.b.word, n * sizeof(int), hipMemcpyDeviceToHost));
    return VO_OK;
}

extern "C" int vo_places_open(vo_ctx* ctx, int capacity)
{
    if (!ctx) return VO_ERR_INVALID;
    if (!ctx->vocab.valid) FAIL(VO_ERR_INVALID, "vo_places_open: there is no vocabulary (vo_vocab_train, vo_vocab_set)");
    if (capacity < 1 || capacity > VO_PLACES_MAX_ENTRIES) FAIL(VO_ERR_INVALID, "vo_places_open: 1 <= capacity <= %d, got %d", VO_PLACES_MAX_ENTRIES, capacity);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->places = PlacesState();
    PlacesState& P = ctx->places;
    const size_t n = (size_t)capacity, K = (size_t)ctx->vocab.K;
    HIPCHK(P.mem.alloc(&P.hist, n * K)); HIPCHK(P.mem.alloc(&P.sum, n)); HIPCHK(P.mem.alloc(&P.id, n));
    P.capacity = capacity; P.n = 0; P.K = ctx->vocab.K; P.open = true;
    return VO_OK;
}

extern "C" int vo_places_add(vo_ctx* ctx, const int32_t* slots, int F, const int32_t* ids, int32_t* first_entry)
{
    if (!ctx) return VO_ERR_INVALID;
    const Batch b = batch(ctx);
    if (!b.ready) FAIL(VO_ERR_NOT_CONFIGURED, "vo_places_add: vo_batch_configure[_sift] has not been called");
    PlacesState& P = ctx->places;
    if (!P.open || !ctx->vocab.valid) FAIL(VO_ERR_INVALID, "vo_places_add: no index is open (vo_places_open)");
    if (F > 0 && !ids) FAIL(VO_ERR_INVALID, "bad arguments");
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int> cnt;
    int rc = places_slots_check(ctx, b, slots, F, "vo_places_add", &cnt); if (rc) return rc;
    if (F > P.capacity - P.n) FAIL(VO_ERR_UNSUPPORTED, "vo_places_add: %d more entries do not fit an index of %d holding %d", F, P.capacity, P.n);
    if (first_entry) *first_entry = P.n;
    if (F == 0) return VO_OK;
    const VocabBuf& vb = ctx->vocab.b;
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(vb.ids, ids, (size_t)F * sizeof(int), hipMemcpyHostToDevice, s));
    rc = quantise(ctx, b, slots, F); if (rc) return rc;
    { StageTimer t(ctx, ST_MISC); launch_places_hist(s, vb, F, b.kp_count, b.kp_cap, P.hist + (size_t)P.n * P.K, P.sum + P.n, P.id + P.n); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    P.n += F;
    return VO_OK;
}

extern "C" int vo_places_add_hist(vo_ctx* ctx, const uint8_t* hist, const int32_t* ids, int n, int32_t* first_entry)
{
    if (!ctx) return VO_ERR_INVALID;
    PlacesState& P = ctx->places;
    if (!P.open) FAIL(VO_ERR_INVALID, "vo_places_add_hist: no index is open (vo_places_open)");
    if (n < 0 || (n > 0 && (!hist || !ids))) FAIL(VO_ERR_INVALID, "bad arguments");
    if (n > P.capacity - P.n) FAIL(VO_ERR_UNSUPPORTED, "vo_places_add_hist: %d more entries do not fit an index of %d holding %d", n, P.capacity, P.n);
    if (first_entry) *first_entry = P.n;
    if (n == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(P.hist + (size_t)P.n * P.K, hist, (size_t)n * P.K, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(P.id + P.n, ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_MISC); launch_places_sums(s, P.hist + (size_t)P.n * P.K, P.K, n, P.sum + P.n); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    P.n += n;
    return VO_OK;
}

extern "C" int vo_places_entries(vo_ctx* ctx, int first, int n, uint8_t* hist, int32_t* sum, int32_t* ids)
{
    if (!ctx) return VO_ERR_INVALID;
    const PlacesState& P = ctx->places;
    if (!P.open) FAIL(VO_ERR_INVALID, "vo_places_entries: no index is open (vo_places_open)");
    if (first < 0 || n < 0 || first > P.n || n > P.n - first) FAIL(VO_ERR_INVALID, "vo_places_entries: entries %d .. %d of %d", first, first + n - 1, P.n);
    if (n == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (hist) HIPCHK(hipMemcpy(hist, P.hist + (size_t)first * P.K, (size_t)n * P.K, hipMemcpyDeviceToHost));
    if (sum) HIPCHK(hipMemcpy(sum, P.sum + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    if (ids) HIPCHK(hipMemcpy(ids, P.id + first, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return VO_OK;
}

extern "C" int vo_places_size(vo_ctx* ctx, int32_t* n, int32_t* K)
{
    if (!ctx) return VO_ERR_INVALID;
    const PlacesState& P = ctx->places;
    if (!P.open) FAIL(VO_ERR_INVALID, "vo_places_size: no index is open (vo_places_open)");
    if (n) *n = P.n;
    if (K) *K = P.K;
    return VO_OK;
}

extern "C" int vo_places_query(vo_ctx* ctx, const int32_t* entries, int Q, const vo_places_opts* o, int32_t* out_entry, int32_t* out_shared)
{
    if (!ctx) return VO_ERR_INVALID;
    const PlacesState& P = ctx->places;
    if (!P.open) FAIL(VO_ERR_INVALID, "vo_places_query: no index is open (vo_places_open)");
    if (!o) FAIL(VO_ERR_INVALID, "vo_places_query: options are needed");
    if (o->top_k < 1 || o->top_k > VO_PLACES_MAX_TOP_K) FAIL(VO_ERR_INVALID, "vo_places_query: 1 <= top_k <= %d, got %d", VO_PLACES_MAX_TOP_K, (int)o->top_k);
    if (Q < 0 || Q > VO_PLACES_MAX_ENTRIES || (Q > 0 && (!entries || !out_entry || !out_shared)))
        FAIL(VO_ERR_INVALID, "vo_places_query: 0 <= Q <= %d query entries, got %d", VO_PLACES_MAX_ENTRIES, Q);
    for (int q = 0; q < Q; q++) if (entries[q] < 0 || entries[q] >= P.n) FAIL(VO_ERR_INVALID, "vo_places_query: entry %d is not in an index of %d", (int)entries[q], P.n);
    if (Q == 0) return VO_OK;
    HIPCHK(hipSetDevice(ctx->device));
    // the entries are dealt over `splits` workgroups per block of 64 queries, so that about a thousand workgroups exist
    const int qblocks = (Q + 63) / 64, tiles = (P.n + 63) / 64;
    const int splits = std::max(1, std::min(std::min(VO_PLACES_MAX_SPLITS, tiles), (1024 + qblocks - 1) / qblocks));
    const int per_split = (tiles + splits - 1) / splits * 64;
    const size_t k = (size_t)o->top_k, a256 = 255;
    const size_t b_ent = 0, b_part = ((size_t)Q * 4 + a256) & ~a256, b_oe = b_part + (size_t)Q * splits * 16 * 8, b_os = b_oe + (((size_t)Q * k * 4 + a256) & ~a256),
                 bytes = b_os + (size_t)Q * k * 4;
    int rc = ctx->places_work.grow(ctx, bytes); if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint8_t* w = ctx->places_work.p;
    PlacesQuery p;
    p.hist = P.hist; p.sum = P.sum; p.id = P.id; p.n = P.n; p.K = P.K;
    p.qent = (const int*)(w + b_ent); p.Q = Q;
    p.top_k = o->top_k; p.min_gap = o->min_gap; p.min_shared = o->min_shared;
    p.splits = splits; p.per_split = per_split;
    p.part = (unsigned long long*)(w + b_part); p.out_entry = (int*)(w + b_oe); p.out_shared = (int*)(w + b_os);
    HIPCHK(hipMemcpyAsync(w + b_ent, entries, (size_t)Q * sizeof(int), hipMemcpyHostToDevice, s));
    { StageTimer t(ctx, ST_MISC); launch_places_query(s, p); }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_entry, p.out_entry, (size_t)Q * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_shared, p.out_shared, (size_t)Q * k * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (ctx->prof) prof_collect(ctx);
    return VO_OK;
}
