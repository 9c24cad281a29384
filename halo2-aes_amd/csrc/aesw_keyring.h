// aesw_keyring.h -- the scheduled key's round-key slots: the one owner of their state (aesw_ctx::keys) and of the protocol every
// writer (aesw_schedule_key_device) and every reader (a scheduled-key launch, the stream check of the host-pointer path) follows.
// Implemented in aesw_keyring.cpp; no other file names a field of a slot or of the ring.  Not part of the public ABI.
//
// The scheduled key (FixedAes128Config::schedule_key, src/aes128.rs:143-152: `self.keys = Some(..)` replaces the key between
// encrypt calls).  Round keys live in SLOTS of 256 B (176 used); every aesw_schedule_key_device takes the next slot of a small
// ring and every scheduled-key launch bakes the pointer of the slot that is current when it is ENQUEUED, so a launch never sees
// a later key.  A slot is rewritten only behind every launch that reads it: one event per distinct reader stream (re-recorded
// by that stream's later launches, which are ordered behind its earlier ones), all of them waited on by the schedule that
// reuses the slot.  That schedule is also ordered behind the key launch that wrote the slot last, when it ran on another
// stream (its `ready` event).  Slots a hipGraph capture has touched (a captured schedule writes one, a captured launch reads one
// on every replay) are PINNED: the ring never hands them out again.
#pragma once
#include <cstdint>
#include <vector>

// Marks what one translation unit of the library takes from another: hidden, not in the dynamic symbol table.  Defined here, the
// first header aesw_ctx.h includes, for every file of csrc/.
#define AESW_INTERNAL __attribute__((visibility("hidden")))

// Which slot an un-captured schedule writes: slot indices and nothing else -- no HIP call, no ROCm include (tests/test_keyring_policy.py
// compiles this part alone with g++, AESW_KEYRING_POLICY_ONLY defined, and replays scripted sequences against it).  It asks its caller
// whether a slot is pinned (`pinned(i)`) and for a slot nobody has used yet (`fresh(&i)`, 0 = made; another status stops the step
// and is handed back).
struct AESW_INTERNAL KeySlotPolicy {
    std::vector<int> ring;   // the ring: slot indices, at most `size` of them
    std::vector<int> spare;  // slots taken out of the ring when `size` shrank (their readers are still tracked)
    int pos = 0;             // ring position of the slot the last eager schedule wrote
    int size = 4;            // option "key_slots": un-pinned slots the ring cycles through (1 = every schedule waits for all readers)

    // The ring's next slot: spare slots (un-pinned ones; a pinned spare is dropped for good) and fresh ones fill the ring up to
    // `size`, a ring that is too long sheds its tail into `spare`, and an entry a capture has pinned meanwhile is replaced.
    template <class Pinned, class Fresh>
    int next(Pinned &&pinned, Fresh &&fresh, int *out) {
        while ((int)ring.size() > size) { spare.push_back(ring.back()); ring.pop_back(); }
        auto take = [&](int *idx) -> int {
            while (!spare.empty()) {
                const int i = spare.back();
                spare.pop_back();
                if (!pinned(i)) { *idx = i; return 0; }
            }
            return fresh(idx);
        };
        if ((int)ring.size() < size) {
            int idx = -1;
            const int rc = take(&idx);
            if (rc != 0) return rc;
            ring.push_back(idx);
            pos = (int)ring.size() - 1;
        } else {
            pos = (pos + 1) % (int)ring.size();
            if (pinned(ring[pos])) {
                int idx = -1;
                const int rc = take(&idx);
                if (rc != 0) return rc;
                ring[pos] = idx;
            }
        }
        *out = ring[pos];
        return 0;
    }
    // The write into the slot next() chose was never issued: one position back (the ring keeps what it holds), so that a later
    // schedule comes to the slot again with its readers intact.
    void step_back() { pos = (pos + (int)ring.size() - 1) % (int)ring.size(); }
};

#ifndef AESW_KEYRING_POLICY_ONLY
#include <hip/hip_runtime.h>

struct aesw_ctx;

// Every function takes the context the ring is a member of (`&ctx->keys == this`): failures go to its last_error.
struct AESW_INTERNAL KeyRing {
    // One use of a slot, from begin_* to end_*: `d` is the slot's device pointer (176 B of round keys; the first 16 are the key)
    struct Access { int slot = -1; hipStream_t s = nullptr; bool captured = false; uint8_t *d = nullptr; };

    int init(aesw_ctx *ctx);      // aesw_create: the first chunk of slots
    void destroy();               // aesw_destroy, behind hipDeviceSynchronize
    void set_ring_size(int n) { policy.size = n; }  // option "key_slots" (1 ... 64), takes effect with the next schedule
    int ring_size() const { return policy.size; }
    bool has_key() const { return have; }
    // read-only statistics (options of the same names)
    uint64_t key_reader_waits() const { return reader_waits; }  // reader events a schedule had to wait on
    uint64_t key_writer_waits() const { return writer_waits; }  // schedules ordered behind another stream's writer of their slot
    int64_t key_slots_allocated() const { return (int64_t)slots.size(); }
    int64_t key_slots_pinned() const;

    // A key launch on `s` is about to write a slot.  Captured: a fresh slot of its own, pinned (it is written on every replay of the
    // graph, whenever that is).  Eager: the ring's next slot, `s` ordered behind every launch that may still read the slot's previous
    // key and behind the key launch that wrote it last on another stream.  A failure leaves the ring as end_write(failure) does.
    int begin_write(aesw_ctx *ctx, hipStream_t s, Access *w);
    // `launch` is what issuing the key launch returned.  Failure: an eager write keeps the slot's readers and steps the ring back; the
    // status is returned.  Success: the readers' events are free again, `ready` is recorded (eager), the slot is the current key.
    int end_write(aesw_ctx *ctx, const Access &w, hipError_t launch);
    // A launch on `s` is about to read the current key: AESW_ERR_NO_KEY without one, else `s` is ordered behind the key launch that
    // wrote the slot -- same stream: stream order; forked from the capture of the writer's stream: that capture's order; another
    // capture: refused unless the key launch has finished; eager: a wait on `ready`; a slot a captured schedule wrote has no event.
    int begin_read(aesw_ctx *ctx, hipStream_t s, Access *r);
    // The launches issued on r.s since begin_read read r.slot: pinned under capture, else tracked for the schedule that reuses the
    // slot.  May be called again for later launches on r.s while no schedule has come between (the chunks of the stream check).
    int end_read(aesw_ctx *ctx, const Access &r);

private:
    struct Reader { hipStream_t s; hipEvent_t e; };
    struct Slot {
        uint8_t *d = nullptr;
        bool pinned = false;
        bool written = false;        // a key launch has been issued into the slot (`writer` may be the null stream: no marker)
        hipEvent_t ready = nullptr;  // recorded behind the key launch that wrote the slot: launches on other streams wait on it
        hipStream_t writer = nullptr;
        std::vector<Reader> readers;  // launches that may still be reading the slot
    };
    std::vector<Slot> slots;
    std::vector<uint8_t *> chunks;       // hipMalloc'ed backing of the slots (KEY_CHUNK_SLOTS each)
    std::vector<hipEvent_t> event_pool;  // reader events not in use
    KeySlotPolicy policy;
    int cur = -1;  // slot of the current key (-1: none scheduled)
    bool have = false;
    uint64_t reader_waits = 0, writer_waits = 0;

    int new_slot(aesw_ctx *ctx, int *out);
    int track_reader(aesw_ctx *ctx, Slot &sl, hipStream_t s);
    int abandon_write(aesw_ctx *ctx, const Access &w, hipError_t e, const char *what);
};
#endif  // AESW_KEYRING_POLICY_ONLY
