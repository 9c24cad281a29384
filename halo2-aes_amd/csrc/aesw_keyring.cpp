// aesw_keyring.cpp -- the scheduled key's round-key slots (aesw_keyring.h): their memory and events, the write protocol of a
// schedule and the read protocol of a scheduled-key launch.  Host code only.
#include "aesw_ctx.h"

namespace {
constexpr size_t KEY_CHUNK_SLOTS = 16, KEY_SLOT_BYTES = 256, KEY_MAX_READERS = 16;

bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    return cs != hipStreamCaptureStatusNone;
}

// Both streams are being captured into the SAME graph (one forked from the other with an event, like the internal streams of
// the batch entry point from the caller's).
bool same_capture(hipStream_t a, hipStream_t b) {
    hipStreamCaptureStatus sa = hipStreamCaptureStatusNone, sb = hipStreamCaptureStatusNone;
    unsigned long long ia = 0, ib = 0;
    if (hipStreamGetCaptureInfo(a, &sa, &ia) != hipSuccess || hipStreamGetCaptureInfo(b, &sb, &ib) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return sa == hipStreamCaptureStatusActive && sb == hipStreamCaptureStatusActive && ia == ib;
}

// While some stream of this thread is being captured (global mode), allocation calls are refused: run them relaxed.
struct RelaxedCapture {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    bool on;
    RelaxedCapture() { on = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess; if (!on) (void)hipGetLastError(); }
    ~RelaxedCapture() { if (on && hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) (void)hipGetLastError(); }
};
}  // namespace

int KeyRing::init(aesw_ctx *ctx) {
    int first = -1;
    const int rc = new_slot(ctx, &first);
    if (rc == AESW_OK) policy.spare.push_back(first);
    return rc;
}

void KeyRing::destroy() {
    for (auto &sl : slots) {
        if (sl.ready) (void)hipEventDestroy(sl.ready);
        for (auto &r : sl.readers) (void)hipEventDestroy(r.e);
    }
    for (hipEvent_t e : event_pool) (void)hipEventDestroy(e);
    for (uint8_t *c : chunks) (void)hipFree(c);
}

int64_t KeyRing::key_slots_pinned() const {
    int64_t n = 0;
    for (const auto &sl : slots) n += sl.pinned ? 1 : 0;
    return n;
}

// A slot nobody has used yet (fresh memory; a new chunk every KEY_CHUNK_SLOTS slots).
int KeyRing::new_slot(aesw_ctx *ctx, int *out) {
    RelaxedCapture relaxed;
    const size_t used = slots.size();
    if (used == chunks.size() * KEY_CHUNK_SLOTS) {
        uint8_t *c = nullptr;
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void **>(&c), KEY_CHUNK_SLOTS * KEY_SLOT_BYTES));
        chunks.push_back(c);
    }
    Slot sl;
    sl.d = chunks.back() + (used % KEY_CHUNK_SLOTS) * KEY_SLOT_BYTES;
    HIP_TRY(ctx, hipEventCreateWithFlags(&sl.ready, hipEventDisableTiming));
    slots.push_back(sl);
    *out = (int)used;
    return AESW_OK;
}

// An un-captured launch on `s` reads slot `sl`: the schedule that reuses the slot will wait for it.  One event per distinct
// stream: a stream's later record is ordered behind its earlier launches, so re-recording loses nobody.
int KeyRing::track_reader(aesw_ctx *ctx, Slot &sl, hipStream_t s) {
    for (auto &r : sl.readers)
        if (r.s == s) { HIP_TRY(ctx, hipEventRecord(r.e, s)); return AESW_OK; }
    if (sl.readers.size() >= KEY_MAX_READERS) {
        // fold the oldest reader into this stream: `s` waits for it BEHIND the launch just issued, so the event recorded
        // next on `s` stands for both
        HIP_TRY(ctx, hipStreamWaitEvent(s, sl.readers.front().e, 0));
        event_pool.push_back(sl.readers.front().e);
        sl.readers.erase(sl.readers.begin());
    }
    hipEvent_t e = nullptr;
    if (!event_pool.empty()) { e = event_pool.back(); event_pool.pop_back(); }
    else HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const hipError_t rc = hipEventRecord(e, s);
    if (rc != hipSuccess) { event_pool.push_back(e); return fail_hip(ctx, rc, "hipEventRecord(key reader)"); }
    sl.readers.push_back(Reader{s, e});
    return AESW_OK;
}

// An eager schedule that fails before its key launch is issued leaves the slot as it was: keep its readers (still tracked)
// and step the ring back, so that the next schedule comes back to the slot with them intact.  (A captured one keeps its
// pinned slot: nothing hands it out again.)
int KeyRing::abandon_write(aesw_ctx *ctx, const Access &w, hipError_t e, const char *what) {
    if (!w.captured) policy.step_back();
    return fail_hip(ctx, e, what);
}

int KeyRing::begin_write(aesw_ctx *ctx, hipStream_t s, Access *w) {
    w->s = s;
    w->captured = stream_capturing(s);
    if (w->captured) {
        // a captured schedule writes its slot on every replay of the graph, whenever that is: a slot of its own, never reused
        const int rc = new_slot(ctx, &w->slot);
        if (rc != AESW_OK) return rc;
        slots[w->slot].pinned = true;
    } else {
        const int rc = policy.next([&](int i) { return slots[i].pinned; }, [&](int *i) { return new_slot(ctx, i); }, &w->slot);
        if (rc != AESW_OK) return rc;
        // write-after-read: every launch that may still read this slot's previous key, on whatever stream, comes first
        Slot &sl = slots[w->slot];
        for (auto &r : sl.readers) {
            const hipError_t e = hipStreamWaitEvent(s, r.e, 0);
            if (e != hipSuccess) return abandon_write(ctx, *w, e, "hipStreamWaitEvent(key readers)");
            ++reader_waits;
        }
        // write-after-write: the key launch that wrote the slot last may still be queued on its own stream; run behind it, or it
        // lands on top of this key and its older key becomes the current one
        if (sl.written && sl.writer != s) {
            const hipError_t e = hipStreamWaitEvent(s, sl.ready, 0);
            if (e != hipSuccess) return abandon_write(ctx, *w, e, "hipStreamWaitEvent(key writer)");
            ++writer_waits;
        }
    }
    w->d = slots[w->slot].d;
    return AESW_OK;
}

int KeyRing::end_write(aesw_ctx *ctx, const Access &w, hipError_t launch) {
    if (launch != hipSuccess) return abandon_write(ctx, w, launch, "launch_key");
    Slot &sl = slots[w.slot];
    sl.written = true;
    if (!w.captured) {
        // the new key is issued behind every earlier reader: their events are free again
        for (auto &r : sl.readers) event_pool.push_back(r.e);
        sl.readers.clear();
        // a later encrypt on ANOTHER stream (the host-pointer entry points use the context's own) waits for these round keys
        HIP_TRY(ctx, hipEventRecord(sl.ready, w.s));
    }
    sl.writer = w.s;
    cur = w.slot;
    have = true;
    return AESW_OK;
}

int KeyRing::begin_read(aesw_ctx *ctx, hipStream_t s, Access *r) {
    if (!have) return AESW_ERR_NO_KEY;  // "Keys should be scheduled", src/aes128.rs:170
    Slot &sl = slots[cur];
    r->slot = cur;
    r->s = s;
    r->d = sl.d;
    r->captured = stream_capturing(s);
    if (s == sl.writer) return AESW_OK;  // stream order
    // the round keys were written on another stream: order the launch behind them
    if (r->captured && same_capture(s, sl.writer)) {
        // `s` was forked (with an event) from the capture on the key's own stream -- the internal streams of the batch entry
        // point and of "split_small" are: whatever ordered the key in front of that capture orders it in front of `s` too.
        // (Asking the key's event would be an error here: its stream is the one being captured.)
    } else if (r->captured) {
        // a captured launch cannot take a dependency on work outside its graph.  If the key launch has already finished,
        // there is nothing to depend on; otherwise refuse instead of dropping the wait silently
        RelaxedCapture relaxed;
        const bool done = !sl.pinned && hipEventQuery(sl.ready) == hipSuccess;
        (void)hipGetLastError();
        if (!done) {
            ctx->last_error = "scheduled-key encrypt captured on a stream other than the one aesw_schedule_key_device ran on, "
                              "and the key launch has not finished (or was itself captured): synchronise first, or capture both on one stream";
            return AESW_ERR_INVALID_ARG;
        }
    } else if (!sl.pinned) {
        HIP_TRY(ctx, hipStreamWaitEvent(s, sl.ready, 0));
    }  // (a slot written by a captured schedule has no event: the caller orders its graph launches, include/aesw.h)
    return AESW_OK;
}

int KeyRing::end_read(aesw_ctx *ctx, const Access &r) {
    Slot &sl = slots[r.slot];
    if (r.captured) { sl.pinned = true; return AESW_OK; }  // read on every replay of the graph, whenever that is: the ring never reuses the slot
    return track_reader(ctx, sl, r.s);
}
