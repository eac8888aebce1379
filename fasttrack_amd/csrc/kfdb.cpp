// KeyFrameDatabase (reference src/KeyFrameDatabase.cc) as a device-resident object: add (:39-45), erase (:47-66), clear (:68-72)
// and the two queries that have a caller, DetectNBestCandidates (:604-730) and DetectRelocalizationCandidates (:733-845), with
// L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  There is no inverted file: a wave per stored keyframe
// intersects two sorted word lists (kernels_kfdb.hip), so add is an append and erase a tombstone.
// A HANDLE is the add sequence number of a keyframe; a ROW is its place in the storage.  Rows are in handle order at all times -
// an append keeps it, and growth and compaction copy the live rows in row order - so the insertion order of every word's list in
// the reference is the row order here, and the order of lKFsSharingWords is ascending (first shared word, row).
// ft_kfdb_score is one block up (call slot, query, connected rows), TWO launches whatever the number of keyframes or words,
// the call's records and the state of the query's kind down, one wait.  The state comes down whole (16 bytes per row) into
// the database's pinned mirror: the selection calls (:671-729, :792-844) read stamps and stored scores there and touch no
// device memory.
#include <set>

#include "search_host.h"

struct ft_kfdb {
    ft_context *ctx = nullptr;
    // storage: word ids and values apart (the counting pass reads ids only), rows, and per kind the state with its pinned mirror
    unsigned *d_ids = nullptr, *d_rowStart = nullptr;
    double *d_vals = nullptr;
    int *d_rowLen = nullptr;
    FtKfdbState *d_state[2] = {nullptr, nullptr}, *h_state[2] = {nullptr, nullptr};
    size_t wordCap = 0, rowCap = 0;
    size_t usedWords = 0, deadWords = 0;  // words of all rows / of the erased ones
    std::vector<unsigned> rowStart;
    std::vector<int> rowLen;     // as added (an erased row keeps its length here; on the device it is 0)
    std::vector<int> rowHandle;  // -1: erased
    std::vector<int> rowOf;      // [handle - handleBase] -> row, -1: erased
    int handleBase = 0;          // handles below it are gone (clear, compaction of a prefix)
    int nextHandle = 0, nLive = 0;
};

namespace {

void freeStorage(ft_kfdb *db) {
    hipFree(db->d_ids);
    hipFree(db->d_vals);
    hipFree(db->d_rowStart);
    hipFree(db->d_rowLen);
    for (int k = 0; k < 2; k++) {
        hipFree(db->d_state[k]);
        hipHostFree(db->h_state[k]);
        db->d_state[k] = db->h_state[k] = nullptr;
    }
    db->d_ids = db->d_rowStart = nullptr;
    db->d_vals = nullptr;
    db->d_rowLen = nullptr;
    db->wordCap = db->rowCap = 0;
}

inline int rowOfHandle(const ft_kfdb *db, int handle) {
    if (handle < db->handleBase || handle >= db->nextHandle) return -1;
    return db->rowOf[handle - db->handleBase];
}

// The live rows, in row order, into storage of wordCap words and rowCap rows (growth by doubling, compaction; also the first
// allocation).  The words move on the device (k_kfdb_move), the state through its mirror, which holds what the device holds.
int rebuild(ft_kfdb *db, size_t wordCap, size_t rowCap) {
    ft_context *ctx = db->ctx;
    ft_kfdb n;  // the new storage; freed on an error
    n.wordCap = wordCap;
    n.rowCap = rowCap;
    struct Guard {
        ft_kfdb *p;
        ~Guard() { if (p) freeStorage(p); }
    } guard{&n};
    FT_HIP(hipMalloc((void **)&n.d_ids, 4 * wordCap));
    FT_HIP(hipMalloc((void **)&n.d_vals, 8 * wordCap));
    FT_HIP(hipMalloc((void **)&n.d_rowStart, 4 * rowCap));
    FT_HIP(hipMalloc((void **)&n.d_rowLen, 4 * rowCap));
    for (int k = 0; k < 2; k++) {
        FT_HIP(hipMalloc((void **)&n.d_state[k], sizeof(FtKfdbState) * rowCap));
        FT_HIP(hipHostMalloc((void **)&n.h_state[k], sizeof(FtKfdbState) * rowCap, hipHostMallocDefault));
        memset(n.h_state[k], 0, sizeof(FtKfdbState) * rowCap);
    }
    std::vector<int> map;
    size_t words = 0;
    for (size_t r = 0; r < db->rowHandle.size(); r++) {
        if (db->rowHandle[r] < 0) continue;
        const size_t to = map.size();
        map.push_back((int)r);
        n.rowStart.push_back((unsigned)words);
        n.rowLen.push_back(db->rowLen[r]);
        n.rowHandle.push_back(db->rowHandle[r]);
        for (int k = 0; k < 2; k++) n.h_state[k][to] = db->h_state[k][r];
        words += (size_t)db->rowLen[r];
    }
    const size_t nRows = map.size();
    hipStream_t st = ctx->stream;
    if (nRows) {
        const int rc = ft_ensure_scratch(ctx, 4 * nRows, 4 * nRows);
        if (rc != FT_OK) return rc;
        memcpy(ctx->scratchPin, map.data(), 4 * nRows);
        FT_HIP(hipMemcpyAsync(ctx->scratchDev, ctx->scratchPin, 4 * nRows, hipMemcpyHostToDevice, st));
        FT_HIP(hipMemcpyAsync(n.d_rowStart, n.rowStart.data(), 4 * nRows, hipMemcpyHostToDevice, st));
        FT_HIP(hipMemcpyAsync(n.d_rowLen, n.rowLen.data(), 4 * nRows, hipMemcpyHostToDevice, st));
        for (int k = 0; k < 2; k++)
            FT_HIP(hipMemcpyAsync(n.d_state[k], n.h_state[k], sizeof(FtKfdbState) * nRows, hipMemcpyHostToDevice, st));
        const int rcl = ft_launch_kfdb_move(st, db->d_ids, db->d_vals, db->d_rowStart, (const int *)ctx->scratchDev, n.d_ids, n.d_vals,
                                            n.d_rowStart, n.d_rowLen, (int)nRows);
        const hipError_t e = hipStreamSynchronize(st);  // (the vectors above are read by the copies until here)
        if (rcl != FT_OK) return rcl;
        FT_HIP(e);
    }
    // handles below the first live one are gone for good
    const int base = nRows ? n.rowHandle[0] : db->nextHandle;
    std::vector<int> rowOf((size_t)(db->nextHandle - base), -1);
    for (size_t r = 0; r < nRows; r++) rowOf[n.rowHandle[r] - base] = (int)r;
    freeStorage(db);
    db->d_ids = n.d_ids;
    db->d_vals = n.d_vals;
    db->d_rowStart = n.d_rowStart;
    db->d_rowLen = n.d_rowLen;
    for (int k = 0; k < 2; k++) db->d_state[k] = n.d_state[k], db->h_state[k] = n.h_state[k];
    db->wordCap = wordCap;
    db->rowCap = rowCap;
    guard.p = nullptr;
    db->rowStart.swap(n.rowStart);
    db->rowLen.swap(n.rowLen);
    db->rowHandle.swap(n.rowHandle);
    db->rowOf.swap(rowOf);
    db->handleBase = base;
    db->usedWords = words;
    db->deadWords = 0;
    return FT_OK;
}

inline size_t doubled(size_t cap, size_t need, size_t least) {
    size_t c = std::max(cap, least);
    while (c < need) c *= 2;
    return c;
}

const char *const KIND_ERR = ": kind is 0 (place recognition) or 1 (relocalisation)";

// :675-700 / :796-821 for one scored keyframe: the accumulated score and pBestKF with its map
struct Acc {
    float score;
    int handle, map;
};
int accumulate(const ft_kfdb *db, const char *fn, int kind, long long query_id, int n_scored, const int *scored_handles,
               const float *scored_scores, const int *neigh_offsets, const int *neigh_handles, const int *scored_map,
               const int *neigh_map, std::vector<Acc> &out, float *bestAcc) {
    FT_REQUIRE(n_scored >= 0, std::string(fn) + ": n_scored < 0");
    FT_REQUIRE(n_scored == 0 || (scored_handles && scored_scores && neigh_offsets && scored_map), std::string(fn) + ": null argument");
    FT_REQUIRE(n_scored == 0 || neigh_offsets[0] == 0, std::string(fn) + ": neigh_offsets[0] != 0");
    for (int i = 0; i < n_scored; i++) {
        FT_REQUIRE(neigh_offsets[i + 1] >= neigh_offsets[i], std::string(fn) + ": neigh_offsets decreases at keyframe " + std::to_string(i));
        FT_REQUIRE(rowOfHandle(db, scored_handles[i]) >= 0, std::string(fn) + ": scored handle " + std::to_string(scored_handles[i]) + " is not in the database");
    }
    const int total = n_scored ? neigh_offsets[n_scored] : 0;
    FT_REQUIRE(total == 0 || (neigh_handles && neigh_map), std::string(fn) + ": null neighbour arrays");
    for (int k = 0; k < total; k++)
        FT_REQUIRE(rowOfHandle(db, neigh_handles[k]) >= 0, std::string(fn) + ": neighbour handle " + std::to_string(neigh_handles[k]) + " is not in the database");
    out.clear();
    float best = 0;
    for (int i = 0; i < n_scored; i++) {
        float bestScore = scored_scores[i], accScore = bestScore;
        Acc a{0.f, scored_handles[i], scored_map[i]};
        for (int k = neigh_offsets[i]; k < neigh_offsets[i + 1]; k++) {
            const FtKfdbState &S = db->h_state[kind][rowOfHandle(db, neigh_handles[k])];
            if (S.stamp != query_id) continue;
            accScore += S.score;
            if (S.score > bestScore) {
                a.handle = neigh_handles[k];
                a.map = neigh_map[k];
                bestScore = S.score;
            }
        }
        a.score = accScore;
        out.push_back(a);
        if (accScore > best) best = accScore;
    }
    *bestAcc = best;
    return FT_OK;
}

}  // namespace

extern "C" {

int ft_kfdb_create(ft_context *ctx, int scoring, ft_kfdb **out) {
    FT_REQUIRE(ctx && out, "ft_kfdb_create: null argument");
    FT_REQUIRE(scoring == 0, "ft_kfdb_create: scoring " + std::to_string(scoring) + " is not implemented: only 0 (L1_NORM, what ORBvoc uses) is");
    int rc = ft_set_device(ctx);
    if (rc != FT_OK) return rc;
    ft_kfdb *db = new ft_kfdb;
    db->ctx = ctx;
    ctx->liveObjects++;
    *out = db;
    return FT_OK;
}

int ft_kfdb_destroy(ft_kfdb *db) {
    if (!db) return FT_OK;
    ft_set_device(db->ctx);
    {
        std::lock_guard<std::mutex> lk(db->ctx->matchMutex);
        hipStreamSynchronize(db->ctx->stream);
        freeStorage(db);
    }
    db->ctx->liveObjects--;
    delete db;
    return FT_OK;
}

int ft_kfdb_add(ft_kfdb *db, int n, const int *bow_offsets, const unsigned *bow_ids, const double *bow_values, int *handles_out) {
    const char *const FN = "ft_kfdb_add";
    FT_REQUIRE(db && n >= 0, std::string(FN) + ": null database or n < 0");
    if (n == 0) return FT_OK;
    FT_REQUIRE(bow_offsets && handles_out, std::string(FN) + ": null argument");
    FT_REQUIRE(bow_offsets[0] == 0, std::string(FN) + ": bow_offsets[0] != 0");
    for (int k = 0; k < n; k++)
        FT_REQUIRE(bow_offsets[k + 1] >= bow_offsets[k], std::string(FN) + ": bow_offsets decreases at keyframe " + std::to_string(k));
    const size_t total = (size_t)bow_offsets[n];
    FT_REQUIRE(total == 0 || (bow_ids && bow_values), std::string(FN) + ": null bow_ids or bow_values");
    for (int k = 0; k < n; k++)
        for (int i = bow_offsets[k]; i < bow_offsets[k + 1]; i++) {
            FT_REQUIRE(bow_ids[i] != FT_KFDB_NOT_LISTED, std::string(FN) + ": word id 0xffffffff is reserved");
            FT_REQUIRE(i == bow_offsets[k] || bow_ids[i] > bow_ids[i - 1],
                       std::string(FN) + ": the word ids of keyframe " + std::to_string(k) + " are not strictly ascending");
        }
    FT_REQUIRE(db->nextHandle <= INT_MAX - n, std::string(FN) + ": out of handles");
    int rc = ft_set_device(db->ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(db->ctx->matchMutex);
    const size_t rows = db->rowHandle.size();
    if (db->usedWords + total > db->wordCap || rows + (size_t)n > db->rowCap) {
        // the dead rows leave on the way; what is needed is what the live rows and the new ones hold
        const size_t needWords = db->usedWords - db->deadWords + total, needRows = (size_t)db->nLive + (size_t)n;
        if (needWords >= 0xffffffffull) {
            ft_set_error(std::string(FN) + ": a database holds fewer than 2^32 words");
            return FT_ERR_CAPACITY;
        }
        rc = rebuild(db, doubled(db->wordCap, needWords, 4096), doubled(db->rowCap, needRows, 64));
        if (rc != FT_OK) return rc;
    }
    const size_t r0 = db->rowHandle.size();
    std::vector<unsigned> start((size_t)n);
    std::vector<int> len((size_t)n);
    for (int k = 0; k < n; k++) {
        start[k] = (unsigned)(db->usedWords + (size_t)bow_offsets[k]);
        len[k] = bow_offsets[k + 1] - bow_offsets[k];
    }
    if (total) {
        FT_HIP(hipMemcpy(db->d_ids + db->usedWords, bow_ids, 4 * total, hipMemcpyHostToDevice));
        FT_HIP(hipMemcpy(db->d_vals + db->usedWords, bow_values, 8 * total, hipMemcpyHostToDevice));
    }
    FT_HIP(hipMemcpy(db->d_rowStart + r0, start.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    FT_HIP(hipMemcpy(db->d_rowLen + r0, len.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
    for (int k = 0; k < 2; k++) {  // mn*Query = 0, mn*Words = 0, m*Score = 0 (KeyFrame.cc:33-34)
        memset(db->h_state[k] + r0, 0, sizeof(FtKfdbState) * (size_t)n);
        FT_HIP(hipMemset(db->d_state[k] + r0, 0, sizeof(FtKfdbState) * (size_t)n));
    }
    for (int k = 0; k < n; k++) {
        db->rowStart.push_back(start[k]);
        db->rowLen.push_back(len[k]);
        db->rowHandle.push_back(db->nextHandle);
        db->rowOf.push_back((int)(r0 + (size_t)k));
        handles_out[k] = db->nextHandle++;
    }
    db->usedWords += total;
    db->nLive += n;
    return FT_OK;
}

int ft_kfdb_erase(ft_kfdb *db, int n, const int *handles) {
    const char *const FN = "ft_kfdb_erase";
    FT_REQUIRE(db && n >= 0 && (n == 0 || handles), std::string(FN) + ": null argument or n < 0");
    if (n == 0) return FT_OK;
    std::set<int> seen;
    for (int k = 0; k < n; k++)
        FT_REQUIRE(rowOfHandle(db, handles[k]) >= 0 && seen.insert(handles[k]).second,
                   std::string(FN) + ": handle " + std::to_string(handles[k]) + " is unknown or already erased");
    int rc = ft_set_device(db->ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(db->ctx->matchMutex);
    int lo = INT_MAX, hi = -1;
    for (int k = 0; k < n; k++) {
        const int r = rowOfHandle(db, handles[k]);
        db->rowOf[handles[k] - db->handleBase] = -1;
        db->rowHandle[r] = -1;
        db->deadWords += (size_t)db->rowLen[r];
        db->nLive--;
        lo = std::min(lo, r);
        hi = std::max(hi, r);
    }
    if (2 * db->deadWords > db->usedWords) {  // dead words exceed half of the stored words: compact, in handle order
        rc = rebuild(db, db->wordCap, db->rowCap);
        if (rc == FT_OK) db->ctx->addStat("kfdb.compactions", 0.0);
        return rc;
    }
    // the tombstone: length 0 on the device for the span of rows the call touched
    std::vector<int> len((size_t)(hi - lo + 1));
    for (int r = lo; r <= hi; r++) len[r - lo] = db->rowHandle[r] < 0 ? 0 : db->rowLen[r];
    FT_HIP(hipMemcpy(db->d_rowLen + lo, len.data(), 4 * len.size(), hipMemcpyHostToDevice));
    return FT_OK;
}

int ft_kfdb_clear(ft_kfdb *db) {
    FT_REQUIRE(db, "ft_kfdb_clear: null database");
    int rc = ft_set_device(db->ctx);
    if (rc != FT_OK) return rc;
    std::lock_guard<std::mutex> lk(db->ctx->matchMutex);
    // the storage stays; nothing of it is read again: every row is gone, and add writes a row before it counts
    db->rowStart.clear();
    db->rowLen.clear();
    db->rowHandle.clear();
    db->rowOf.clear();
    db->handleBase = db->nextHandle;
    db->usedWords = db->deadWords = 0;
    db->nLive = 0;
    return FT_OK;
}

int ft_kfdb_size(const ft_kfdb *db, int *n_live, long long *n_words) {
    FT_REQUIRE(db, "ft_kfdb_size: null database");
    if (n_live) *n_live = db->nLive;
    if (n_words) *n_words = (long long)(db->usedWords - db->deadWords);
    return FT_OK;
}

int ft_kfdb_state(const ft_kfdb *db, int kind, int n, const int *handles, long long *stamps, int *words, float *scores) {
    const char *const FN = "ft_kfdb_state";
    FT_REQUIRE(db && n >= 0 && (n == 0 || handles), std::string(FN) + ": null argument or n < 0");
    FT_REQUIRE(kind == 0 || kind == 1, std::string(FN) + KIND_ERR);
    for (int k = 0; k < n; k++)
        FT_REQUIRE(rowOfHandle(db, handles[k]) >= 0, std::string(FN) + ": handle " + std::to_string(handles[k]) + " is not in the database");
    for (int k = 0; k < n; k++) {
        const FtKfdbState &S = db->h_state[kind][rowOfHandle(db, handles[k])];
        if (stamps) stamps[k] = S.stamp;
        if (words) words[k] = S.words;
        if (scores) scores[k] = S.score;
    }
    return FT_OK;
}

int ft_kfdb_score(ft_kfdb *db, int kind, long long query_id, int n_words, const unsigned *ids, const double *values, int n_connected,
                  const int *connected_handles, int *n_sharing, int *max_common_words, int *min_common_words, int *n_scored,
                  int *scored_handles, int *scored_words, float *scored_scores, double *raw_scores) {
    const char *const FN = "ft_kfdb_score";
    FT_REQUIRE(db && n_sharing && max_common_words && min_common_words && n_scored, std::string(FN) + ": null argument");
    FT_REQUIRE(kind == 0 || kind == 1, std::string(FN) + KIND_ERR);
    FT_REQUIRE(n_words >= 0 && n_connected >= 0, std::string(FN) + ": negative count");
    FT_REQUIRE(n_words == 0 || (ids && values), std::string(FN) + ": null ids or values with n_words > 0");
    FT_REQUIRE(n_connected == 0 || connected_handles, std::string(FN) + ": null connected_handles with n_connected > 0");
    FT_REQUIRE(kind == 0 || n_connected == 0, std::string(FN) + ": the relocalisation query has no connected set");
    if (n_words > FT_KFDB_MAX_QUERY_WORDS) {
        ft_set_error(std::string(FN) + ": a query of " + std::to_string(n_words) + " words, more than the " +
                     std::to_string(FT_KFDB_MAX_QUERY_WORDS) + " a query may hold");
        return FT_ERR_CAPACITY;
    }
    for (int i = 0; i < n_words; i++)
        FT_REQUIRE(ids[i] != FT_KFDB_NOT_LISTED && (i == 0 || ids[i] > ids[i - 1]), std::string(FN) + ": the query's word ids are not strictly ascending");
    std::vector<int> conn((size_t)n_connected);
    for (int k = 0; k < n_connected; k++) {
        conn[k] = rowOfHandle(db, connected_handles[k]);
        FT_REQUIRE(conn[k] >= 0, std::string(FN) + ": connected handle " + std::to_string(connected_handles[k]) + " is not live");
    }
    *n_sharing = *max_common_words = *min_common_words = *n_scored = 0;
    const int nRows = (int)db->rowHandle.size();
    if (n_words == 0 || db->usedWords == db->deadWords) return FT_OK;  // nothing can share a word (:637-638, :758-759)
    FT_REQUIRE(scored_handles && scored_words && scored_scores, std::string(FN) + ": null output arrays");
    std::sort(conn.begin(), conn.end());
    int rc = ft_set_device(db->ctx);
    if (rc != FT_OK) return rc;
    ft_context *ctx = db->ctx;
    std::lock_guard<std::mutex> lk(ctx->matchMutex);
    FtTimer tAll;
    const size_t nr = (size_t)nRows, nq = (size_t)n_words, nc = (size_t)n_connected;
    Arena a;
    const size_t oIds = a.take(4 * nq);
    const size_t oVals = a.take(8 * nq);
    const size_t oConn = a.take(4 * nc);
    const size_t oSlot = a.take(64);
    const size_t inputEnd = a.off;
    const size_t oRecs = a.take(sizeof(FtKfdbRec) * nr);
    const size_t oRaw = a.take(8 * nr);
    const size_t outputEnd = a.off;
    const size_t oFirst = a.take(4 * nr);
    if (a.off >= 0xffffffffull) {
        ft_set_error(std::string(FN) + ": the call's arena exceeds 4 GB");
        return FT_ERR_CAPACITY;
    }
    rc = ft_ensure_scratch(ctx, a.off, outputEnd);
    if (rc != FT_OK) return rc;
    uint8_t *pin = (uint8_t *)ctx->scratchPin, *dev = (uint8_t *)ctx->scratchDev;
    memcpy(pin + oIds, ids, 4 * nq);
    memcpy(pin + oVals, values, 8 * nq);
    if (nc) memcpy(pin + oConn, conn.data(), 4 * nc);
    memset(pin + oSlot, 0, 64);
    FtKfdbCall T;
    memset(&T, 0, sizeof T);
    T.ids = db->d_ids;
    T.vals = db->d_vals;
    T.rowStart = db->d_rowStart;
    T.rowLen = db->d_rowLen;
    T.state = db->d_state[kind];
    T.nRows = nRows;
    T.arena = dev;
    T.slot = (unsigned)oSlot;
    T.qIds = (unsigned)oIds;
    T.qVals = (unsigned)oVals;
    T.connected = (unsigned)oConn;
    T.recs = (unsigned)oRecs;
    T.raw = (unsigned)oRaw;
    T.first = (unsigned)oFirst;
    T.nQuery = n_words;
    T.nConnected = n_connected;
    T.queryId = query_id;
    hipStream_t st = ctx->stream;
    CallEventTimer own;
    CallScope C{ctx, st, dev, pin, own.evt};
    C.up(0, inputEnd);  // one copy: the block is contiguous
    C.launch("kernel.kfdb_count", [&] { return ft_launch_kfdb_count(st, T); });
    C.launch("kernel.kfdb_score", [&] { return ft_launch_kfdb_score(st, T); });
    if (C.rc == FT_OK)  // the state of this kind into its mirror: what the selection calls read
        C.hip(hipMemcpyAsync(db->h_state[kind], db->d_state[kind], sizeof(FtKfdbState) * nr, hipMemcpyDeviceToHost, st), "hipMemcpyAsync (state down)");
    rc = C.down(oSlot, outputEnd);
    if (rc != FT_OK) return rc;
    const int *slot = (const int *)(pin + oSlot);
    const int nScored = slot[2];
    *n_sharing = slot[0];
    *max_common_words = slot[1];
    *min_common_words = slot[0] ? (int)(slot[1] * 0.8f) : 0;
    *n_scored = nScored;
    // the order of lKFsSharingWords: first encounter, walking the query's words ascending and each word's list in insertion order
    const FtKfdbRec *recs = (const FtKfdbRec *)(pin + oRecs);
    const double *raw = (const double *)(pin + oRaw);
    std::vector<int> order((size_t)nScored);
    for (int k = 0; k < nScored; k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](int x, int y) {
        return (unsigned)recs[x].first != (unsigned)recs[y].first ? (unsigned)recs[x].first < (unsigned)recs[y].first : recs[x].row < recs[y].row;
    });
    for (int k = 0; k < nScored; k++) {
        const FtKfdbRec &R = recs[order[k]];
        scored_handles[k] = db->rowHandle[R.row];
        scored_words[k] = R.words;
        scored_scores[k] = R.score;
        if (raw_scores) raw_scores[k] = raw[order[k]];
    }
    ctx->addStat("kfdb_score.total", tAll.ms());
    ctx->addStat("kfdb_score.launches", C.launches);
    return FT_OK;
}

int ft_kfdb_select_n_best(const ft_kfdb *db, long long query_id, int n_scored, const int *scored_handles, const float *scored_scores,
                          const int *neigh_offsets, const int *neigh_handles, const int *scored_map, const int *neigh_map, int query_map,
                          int n_bad_maps, const int *bad_maps, int n_candidates, int *loop_out, int *n_loop, int *merge_out, int *n_merge) {
    const char *const FN = "ft_kfdb_select_n_best";
    FT_REQUIRE(db && n_loop && n_merge, std::string(FN) + ": null argument");
    FT_REQUIRE(n_candidates >= 0 && n_bad_maps >= 0 && (n_bad_maps == 0 || bad_maps), std::string(FN) + ": bad n_candidates or bad_maps");
    FT_REQUIRE(n_candidates == 0 || n_scored <= 0 || (loop_out && merge_out), std::string(FN) + ": null output arrays");
    std::vector<Acc> acc;
    float bestAcc = 0;
    const int rc = accumulate(db, FN, 0, query_id, n_scored, scored_handles, scored_scores, neigh_offsets, neigh_handles, scored_map,
                              neigh_map, acc, &bestAcc);
    if (rc != FT_OK) return rc;
    *n_loop = *n_merge = 0;
    // lAccScoreAndMatch.sort(compFirst) (:702): std::list::sort is stable
    std::stable_sort(acc.begin(), acc.end(), [](const Acc &x, const Acc &y) { return x.score > y.score; });
    std::set<int> added;
    int nl = 0, nm = 0;
    for (size_t i = 0; i < acc.size() && (nl < n_candidates || nm < n_candidates); i++) {
        const Acc &A = acc[i];
        if (added.count(A.handle)) continue;
        if (query_map == A.map && nl < n_candidates) loop_out[nl++] = A.handle;
        else if (query_map != A.map && nm < n_candidates && !std::count(bad_maps, bad_maps + n_bad_maps, A.map)) merge_out[nm++] = A.handle;
        added.insert(A.handle);
    }
    *n_loop = nl;
    *n_merge = nm;
    return FT_OK;
}

int ft_kfdb_select_reloc(const ft_kfdb *db, long long query_id, int n_scored, const int *scored_handles, const float *scored_scores,
                         const int *neigh_offsets, const int *neigh_handles, const int *scored_map, const int *neigh_map, int map,
                         int *out, int *n_out) {
    const char *const FN = "ft_kfdb_select_reloc";
    FT_REQUIRE(db && n_out, std::string(FN) + ": null argument");
    FT_REQUIRE(n_scored <= 0 || out, std::string(FN) + ": null output array");
    std::vector<Acc> acc;
    float bestAcc = 0;
    const int rc = accumulate(db, FN, 1, query_id, n_scored, scored_handles, scored_scores, neigh_offsets, neigh_handles, scored_map,
                              neigh_map, acc, &bestAcc);
    if (rc != FT_OK) return rc;
    const float minScoreToRetain = 0.75f * bestAcc;  // :824
    std::set<int> added;
    int n = 0;
    for (const Acc &A : acc) {
        if (!(A.score > minScoreToRetain)) continue;
        if (A.map != map) continue;
        if (added.insert(A.handle).second) out[n++] = A.handle;
    }
    *n_out = n;
    return FT_OK;
}

}  // extern "C"
