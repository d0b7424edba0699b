// stage_check.cpp — the slot protocol of sy_amd/csrc/sydelta_stage.hpp without a GPU.
//
// The HIP calls that StageRing makes are defined here as recorders.  Each appends to one
// in-order log.  hipMemcpyAsync copies nothing when called: it notes destination, source and
// size and checksums the source; the bytes are "in flight" until the stream is known to have
// passed them, which happens when an event recorded behind them is synchronised or when the
// driver drains the stream at the end of its call.  On landing the source is checksummed again
// (a slot rewritten while in flight shows here) and only then copied.
//
// The program drives the ring the way its five users do and checks, for 2, 4 and 8 slots and
// 1, slots, slots + 1 and 3 * slots + 1 uses:
//   * acquire never hands out a slot with bytes in flight, and every landing finds the bytes
//     the upload was queued with; the destination ends up equal to what the host wrote;
//   * every upload is followed by exactly one record of its slot's event on the upload's stream;
//   * the first `slots` uses wait for nothing, use k >= slots waits for the event of slot
//     k % slots, once;
//   * two devices get distinct events, a second call on a device creates none;
//   * the pinned buffer is allocated once across calls and freed with the ring.
// A driver that skips the wait must be caught, or the checks prove nothing: that is tried first.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <set>
#include <vector>

#include "sydelta_stage.hpp"

namespace {

enum Kind { kMemcpy, kRecord, kSync, kWait };
struct Entry {
    Kind kind;
    hipStream_t stream;
    hipEvent_t event;
    uint8_t* dst;
    const uint8_t* src;
    size_t bytes;
    uint64_t sum;
    bool landed;
};
struct Event {
    hipStream_t stream = nullptr;
    size_t upto = 0;  // log entries before this one have been passed when the event completes
};

std::vector<Entry> g_log;
std::deque<Event> g_events;  // never destroyed by the ring: owned here, so no leak is reported
int g_host_allocs = 0, g_host_frees = 0, g_streams = 0, g_failures = 0;

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (!g_failures++) {                           \
                fprintf(stderr, "stage_check: %s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);              \
                fprintf(stderr, "\n");                     \
            }                                              \
        }                                                  \
    } while (0)

uint64_t checksum(const uint8_t* p, size_t n) {
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

// The copies of `stream` among the first `upto` log entries land.
void land(hipStream_t stream, size_t upto) {
    for (size_t i = 0; i < upto; ++i) {
        Entry& e = g_log[i];
        if (e.kind != kMemcpy || e.stream != stream || e.landed) continue;
        CHECK(checksum(e.src, e.bytes) == e.sum, "log entry %zu: the source of an upload changed while in flight", i);
        memcpy(e.dst, e.src, e.bytes);
        e.landed = true;
    }
}
void drain(hipStream_t stream) { land(stream, g_log.size()); }  // the driver's hipStreamSynchronize

bool in_flight(const uint8_t* p, size_t n) {
    for (const Entry& e : g_log)
        if (e.kind == kMemcpy && !e.landed && e.src < p + n && p < e.src + e.bytes) return true;
    return false;
}

}  // namespace

extern "C" {
hipError_t hipHostMalloc(void** p, size_t n, unsigned int) {
    ++g_host_allocs;
    *p = malloc(n ? n : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipHostFree(void* p) {
    ++g_host_frees;
    free(p);
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    CHECK(flags == hipEventDisableTiming, "an event with flags %u", flags);
    g_events.emplace_back();
    *e = (hipEvent_t)&g_events.back();
    return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned int flags) {
    CHECK(flags == hipStreamNonBlocking, "a stream with flags %u", flags);
    *s = (hipStream_t)(uintptr_t)(0x1000 + 16 * ++g_streams);
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    g_log.push_back(Entry{kRecord, s, e, nullptr, nullptr, 0, 0, false});
    Event* ev = (Event*)e;
    ev->stream = s;
    ev->upto = g_log.size();
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e) {
    g_log.push_back(Entry{kSync, nullptr, e, nullptr, nullptr, 0, 0, false});
    const Event* ev = (const Event*)e;
    land(ev->stream, ev->upto);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned int) {
    g_log.push_back(Entry{kWait, s, e, nullptr, nullptr, 0, 0, false});
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* dst, const void* src, size_t n, hipMemcpyKind kind, hipStream_t s) {
    CHECK(kind == hipMemcpyHostToDevice, "a copy of kind %d", (int)kind);
    g_log.push_back(Entry{kMemcpy, s, nullptr, (uint8_t*)dst, (const uint8_t*)src, n, checksum((const uint8_t*)src, n), false});
    return hipSuccess;
}
}

namespace {

using sydelta::StageRing;
const hipStream_t kUser = (hipStream_t)(uintptr_t)0x800;  // the caller's stream

uint8_t pattern(uint64_t call, uint64_t k, size_t i) { return (uint8_t)(call * 131 + k * 29 + i * 7 + (i >> 8) + 1); }

void* acquire(StageRing& r, uint64_t k) {
    void* p = nullptr;
    CHECK(r.acquire(k, &p) == hipSuccess && p, "acquire(%llu) failed", (unsigned long long)k);
    CHECK(!in_flight((const uint8_t*)p, r.slot_bytes()), "acquire(%llu) handed out a slot with bytes in flight",
          (unsigned long long)k);
    return p;
}

// What the log of one call must look like from entry `from` on: `uses` uploads (one or more
// copies each) on `up`, every one followed by one record of its slot's event on `up` (and a
// wait of `waiter` for it); waits for the uses from `slots` on, each for its slot's event, in
// order.  slot_event gets the slots' events.
void check_log(size_t from, uint32_t slots, uint64_t uses, hipStream_t up, hipStream_t waiter, bool acquires,
               std::vector<hipEvent_t>* slot_event) {
    slot_event->resize(slots, nullptr);
    uint64_t use = 0, syncs = 0;
    for (size_t i = from; i < g_log.size(); ++i) {
        const Entry& e = g_log[i];
        if (e.kind == kMemcpy) {
            CHECK(e.stream == up, "entry %zu: an upload on another stream", i);
            size_t j = i + 1;
            while (j < g_log.size() && g_log[j].kind == kMemcpy) ++j;  // the copies of one use
            CHECK(j < g_log.size() && g_log[j].kind == kRecord && g_log[j].stream == up,
                  "entry %zu: an upload is not followed by a record on its stream", i);
            if (j >= g_log.size()) return;
            hipEvent_t& mine = (*slot_event)[use % slots];
            if (!mine) mine = g_log[j].event;
            CHECK(mine == g_log[j].event, "use %llu recorded another event than its slot's", (unsigned long long)use);
            if (waiter)
                CHECK(j + 1 < g_log.size() && g_log[j + 1].kind == kWait && g_log[j + 1].stream == waiter &&
                          g_log[j + 1].event == mine, "use %llu: the kernel stream does not wait for the upload",
                      (unsigned long long)use);
            CHECK(j + 1 >= g_log.size() || g_log[j + 1].kind != kRecord, "use %llu recorded twice", (unsigned long long)use);
            ++use;
            i = j;
        } else if (e.kind == kSync) {
            const uint64_t k = slots + syncs++;  // the use this wait is for
            CHECK(k >= use && k < use + slots, "a wait out of order (for use %llu, at use %llu)", (unsigned long long)k,
                  (unsigned long long)use);
            CHECK(e.event == (*slot_event)[k % slots], "the wait of use %llu is for another slot's event",
                  (unsigned long long)k);
        }
    }
    CHECK(use == uses, "%llu uploads recorded, %llu made", (unsigned long long)use, (unsigned long long)uses);
    const uint64_t want = acquires && uses > slots ? uses - slots : 0;
    CHECK(syncs == want, "%llu waits for %llu uses of %u slots (want %llu)", (unsigned long long)syncs,
          (unsigned long long)uses, slots, (unsigned long long)want);
    std::set<hipEvent_t> distinct(slot_event->begin(), slot_event->end());
    distinct.erase(nullptr);
    CHECK(distinct.size() == std::min<uint64_t>(slots, uses), "slots share an event");
}

struct Call {
    StageRing& r;
    uint32_t slots;
    size_t slot_bytes;
    int device;
    uint64_t call;
    std::vector<uint8_t> dev, want;  // the "device" table and what it must hold
    size_t log0;
    Call(StageRing& r_, uint32_t slots_, size_t slot_bytes_, int device_, uint64_t call_, uint64_t uses)
        : r(r_), slots(slots_), slot_bytes(slot_bytes_), device(device_), call(call_), dev(uses * slot_bytes_, 0),
          want(uses * slot_bytes_, 0), log0(g_log.size()) {
        CHECK(r.open(device, (size_t)slots * slot_bytes) == hipSuccess, "open failed");
        CHECK(r.slot_bytes() == slot_bytes, "slot size %zu, want %zu", r.slot_bytes(), slot_bytes);
    }
    // use k: the slot is filled, `part` of it is meant for the device (two copies, like a slice's two tables)
    void fill(uint64_t k, void* slot, size_t part) {
        uint8_t* h = (uint8_t*)slot;
        for (size_t i = 0; i < slot_bytes; ++i) h[i] = pattern(call, k, i);
        memcpy(want.data() + k * slot_bytes, h, part);
    }
    void copy(uint64_t k, void* slot, size_t part, hipStream_t s) {
        uint8_t* d = dev.data() + k * slot_bytes;
        const uint8_t* h = (const uint8_t*)slot;
        CHECK(hipMemcpyAsync(d, h, part / 2, hipMemcpyHostToDevice, s) == hipSuccess, "copy");
        CHECK(hipMemcpyAsync(d + part / 2, h + part / 2, part - part / 2, hipMemcpyHostToDevice, s) == hipSuccess, "copy");
    }
    void finish(hipStream_t up, hipStream_t user) {
        drain(up);
        drain(user);
        CHECK(dev == want, "device %d, call %llu: the table on the device differs from what the host wrote", device,
              (unsigned long long)call);
        for (const Entry& e : g_log) CHECK(e.kind != kMemcpy || e.landed, "a copy never landed");
    }
};

size_t part_of(uint64_t k, size_t slot_bytes) { return slot_bytes - (k * 24) % (slot_bytes / 2); }  // slices are rarely full

// sydelta_zstd_compress_batch_device's shape without the array: fill, copy, record, one stream.
void drive_plain(StageRing& r, uint32_t slots, size_t sb, int device, uint64_t call, uint64_t uses, bool skip_wait,
                 std::vector<hipEvent_t>* ev) {
    Call c(r, slots, sb, device, call, uses);
    for (uint64_t k = 0; k < uses; ++k) {
        void* slot = skip_wait ? r.base() + (k % slots) * sb : acquire(r, k);
        c.fill(k, slot, part_of(k, sb));
        c.copy(k, slot, part_of(k, sb), kUser);
        CHECK(r.uploaded(k, kUser) == hipSuccess, "uploaded");
    }
    c.finish(kUser, kUser);
    if (!skip_wait) check_log(c.log0, slots, uses, kUser, nullptr, true, ev);
}

// sydelta_apply_delta_batch_device: uploads on the ring's copy stream, the kernels' stream waits.
void drive_copy_stream(StageRing& r, uint32_t slots, size_t sb, int device, uint64_t call, uint64_t uses,
                       std::vector<hipEvent_t>* ev) {
    Call c(r, slots, sb, device, call, uses);
    hipStream_t copy = nullptr;
    CHECK(r.copy_stream(kUser, &copy) == hipSuccess && copy && copy != kUser, "copy_stream");
    const size_t n = g_log.size();  // ready recorded on the caller's stream, the copy stream waits for it
    CHECK(n >= c.log0 + 2 && g_log[n - 2].kind == kRecord && g_log[n - 2].stream == kUser && g_log[n - 1].kind == kWait &&
              g_log[n - 1].stream == copy && g_log[n - 1].event == g_log[n - 2].event, "the copy stream is not ordered");
    for (uint64_t k = 0; k < uses; ++k) {
        void* slot = acquire(r, k);
        c.fill(k, slot, part_of(k, sb));
        c.copy(k, slot, part_of(k, sb), copy);
        CHECK(r.uploaded(k, copy, kUser) == hipSuccess, "uploaded");
    }
    c.finish(copy, kUser);
    check_log(n, slots, uses, copy, kUser, true, ev);
    for (hipEvent_t e : *ev) CHECK(e != g_log[n - 2].event, "a slot shares the copy stream's event");
}

// sydelta_delta_batch_to_json_device: half a ring acquired, filled (by the pool), then uploaded in order.
void drive_half_ring(StageRing& r, uint32_t slots, size_t sb, int device, uint64_t call, uint64_t uses,
                     std::vector<hipEvent_t>* ev) {
    Call c(r, slots, sb, device, call, uses);
    const uint32_t group = slots / 2;
    for (uint64_t j0 = 0; j0 < uses; j0 += group) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(group, uses - j0);
        void* slot[8];
        for (uint32_t k = 0; k < n; ++k) slot[k] = acquire(r, j0 + k);
        for (uint32_t k = n; k-- > 0;) c.fill(j0 + k, slot[k], part_of(j0 + k, sb));  // in any order
        for (uint32_t k = 0; k < n; ++k) {
            c.copy(j0 + k, slot[k], part_of(j0 + k, sb), kUser);
            CHECK(r.uploaded(j0 + k, kUser) == hipSuccess, "uploaded");
        }
    }
    c.finish(kUser, kUser);
    check_log(c.log0, slots, uses, kUser, nullptr, true, ev);
}

// sydelta_zstd_decompress_batch_device: two tables of different element sizes through one count
// of uses; neither length is a multiple of a slot.
struct File { uint64_t a, b; };
struct Base { uint64_t v[5]; };
void drive_arrays(StageRing& r, uint32_t slots, int device, uint64_t uses) {
    const size_t sb = 40 * 16 * 3;  // 120 Files or 48 Bases a slot
    const size_t log0 = g_log.size();
    CHECK(r.open(device, slots * sb) == hipSuccess, "open failed");
    const uint64_t u1 = (uses + 1) / 2, u2 = uses - u1;
    std::vector<File> files(u1 * 120 - 7), d_files(files.size());
    std::vector<Base> bases(u2 ? u2 * 48 - 5 : 0), d_bases(bases.size());
    for (size_t i = 0; i < files.size(); ++i) files[i] = File{i * 3 + 1, ~i};
    for (size_t i = 0; i < bases.size(); ++i) bases[i] = Base{{i, i + 1, i * i, ~i, 7}};
    uint64_t k = 0;
    CHECK(r.upload(files.data(), files.size(), d_files.data(), &k, kUser) == hipSuccess && k == u1, "upload of files");
    CHECK(r.upload(bases.data(), bases.size(), d_bases.data(), &k, kUser) == hipSuccess && k == uses, "upload of bases");
    drain(kUser);
    CHECK(!memcmp(files.data(), d_files.data(), files.size() * sizeof(File)), "the file table arrived changed");
    CHECK(bases.empty() || !memcmp(bases.data(), d_bases.data(), bases.size() * sizeof(Base)), "the bases arrived changed");
    std::vector<hipEvent_t> ev;
    check_log(log0, slots, uses, kUser, nullptr, true, &ev);
    size_t last = 0;  // the tail of the file table is one short copy
    for (size_t i = log0; i < g_log.size(); ++i)
        if (g_log[i].kind == kMemcpy && g_log[i].dst < (uint8_t*)(d_files.data() + d_files.size()) &&
            g_log[i].dst >= (uint8_t*)d_files.data())
            last = g_log[i].bytes;
    CHECK(last == (120 - 7) * sizeof(File), "the last piece of the file table has %zu bytes", last);
}

// sydelta_apply_delta_device: one growing table, up to `slots` batches of any size a call, each
// with its own event; nothing is acquired because nothing is written twice in a call.
void drive_growing() {
    const int a0 = g_host_allocs, f0 = g_host_frees;
    {
        StageRing r(8);
        size_t cap = 0;
        for (size_t need : {(size_t)1000, (size_t)600, (size_t)5000, (size_t)4000}) {
            if (need > cap) cap = need * 5 / 4;
            const size_t log0 = g_log.size(), ev0 = g_events.size();
            CHECK(r.open(0, cap) == hipSuccess, "open failed");
            hipStream_t copy = nullptr;
            CHECK(r.copy_stream(kUser, &copy) == hipSuccess, "copy_stream");
            std::vector<uint8_t> dev(need, 0);
            uint8_t* h = r.base();
            const size_t per = (need + 7) / 8;
            uint64_t j = 0;
            for (size_t i0 = 0; i0 < need; i0 += per, ++j) {
                const size_t n = std::min(per, need - i0);
                for (size_t i = i0; i < i0 + n; ++i) h[i] = pattern(need, j, i);
                CHECK(hipMemcpyAsync(dev.data() + i0, h + i0, n, hipMemcpyHostToDevice, copy) == hipSuccess, "copy");
                CHECK(r.uploaded(j, copy, kUser) == hipSuccess, "uploaded");
            }
            drain(copy);
            drain(kUser);
            CHECK(!memcmp(dev.data(), h, need), "the piece table arrived changed");
            std::vector<hipEvent_t> ev;
            check_log(log0 + 2, 8, j, copy, kUser, false, &ev);
            // the eight batches' events and the copy stream's come with the first call
            CHECK(g_events.size() - ev0 == (need == 1000 ? 9u : 0u), "events created in a later call");
        }
        CHECK(g_host_allocs - a0 == 2 && g_host_frees - f0 == 1, "the table grew %d times, freed %d", g_host_allocs - a0,
              g_host_frees - f0);
    }
    CHECK(g_host_allocs - a0 == 2 && g_host_frees - f0 == 2, "the grown table was not freed with the ring");
}

}  // namespace

int main() {
    // 0. the checks see a driver that does not wait
    {
        StageRing r(2);
        std::vector<hipEvent_t> ev;
        drive_plain(r, 2, 256, 0, 1, 5, true, &ev);
        if (!g_failures) {
            fprintf(stderr, "stage_check: a driver that overwrites a slot in flight was not caught\n");
            return 1;
        }
        g_failures = 0;
        g_log.clear();
    }
    int runs = 0;
    for (uint32_t slots : {2u, 4u, 8u}) {
        const uint64_t counts[] = {1, slots, slots + 1, 3 * slots + 1};
        for (int shape = 0; shape < 4; ++shape) {
            const int a0 = g_host_allocs, f0 = g_host_frees;
            {
                StageRing r(slots);
                const size_t sb = 1536;
                std::vector<hipEvent_t> dev0, dev1, again;
                uint64_t call = 0;
                for (uint64_t uses : counts) {
                    g_log.clear();
                    const size_t e0 = g_events.size();
                    for (int pass = 0; pass < 3; ++pass) {  // device 0, device 1, device 0 again
                        const int device = pass == 1;
                        std::vector<hipEvent_t>& ev = pass == 0 ? dev0 : pass == 1 ? dev1 : again;
                        ev.clear();
                        if (shape == 0) drive_plain(r, slots, sb, device, call, uses, false, &ev);
                        if (shape == 1) drive_copy_stream(r, slots, sb, device, call, uses, &ev);
                        if (shape == 2) drive_half_ring(r, slots, sb, device, call, uses, &ev);
                        if (shape == 3) drive_arrays(r, slots, device, uses);
                        ++call, ++runs;
                    }
                    if (shape == 3) continue;
                    for (uint64_t i = 0; i < std::min<uint64_t>(uses, slots); ++i) {
                        CHECK(dev0[i] == again[i], "a second call on a device uses other events");
                        for (hipEvent_t e : dev1) CHECK(e != dev0[i], "two devices share an event");
                    }
                    // both devices' events come with the first call on each, none later
                    const size_t made = g_events.size() - e0, want = uses == 1 ? 2 * (slots + (shape == 1)) : 0;
                    CHECK(made == want, "%zu events created, want %zu", made, want);
                }
                CHECK(g_host_allocs - a0 == 1 && g_host_frees == f0, "the pinned ring was allocated %d times, freed %d",
                      g_host_allocs - a0, g_host_frees - f0);
            }
            CHECK(g_host_frees - f0 == 1, "the pinned ring was not freed with its owner");
        }
    }
    g_log.clear();
    drive_growing();
    if (g_failures) {
        fprintf(stderr, "stage_check: %d checks failed\n", g_failures);
        return 1;
    }
    printf("stage_check ok: %d calls\n", runs);
    return 0;
}
