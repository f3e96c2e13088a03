// Host-only harness for katsdpimager_amd/csrc/kimg_graph_cache.h (tests/test_graph_cache_host.py
// builds and runs it).  The header is included as it is; the HIP entry points it calls, and
// kimg_capture_stream, are defined HERE as a scripted fake: handles are small heap objects, events
// fire when a case says so, the current device is a variable, and every entry point can be told to
// fail on its n-th call.  No GPU is opened and none is needed.
//
// How the program's own definitions come to be the ones called: it is compiled as HIP for the host
// only and linked without the HIP runtime,
//     hipcc -x hip --offload-host-only -no-hip-rt -I katsdpimager_amd/csrc ...
// so the hip* symbols the header refers to can only be resolved inside the executable -- a missing
// one is a link error, not a call into libamdhip64.  `nm` shows them as defined text symbols
// (T hipEventQuery, ...) and `ldd` lists neither libamdhip64 nor libhsa-runtime64; the pytest file
// asserts both.  (Linked the default way the executable's definitions would still win, symbols of an
// executable coming before those of its libraries, but the runtime would be loaded for nothing.)
//
// Usage: graph_cache_harness [all | threads | <case name>]; exit status 0 = every case passed.
// A failed check prints "FAIL <case><SLOTS> ...".
#include "kimg_graph_cache.h"

#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <map>
#include <random>
#include <set>
#include <thread>
#include <type_traits>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#define HARNESS_ASAN 1
#endif
#endif

// ---- failure reporting ------------------------------------------------------------------------------
static std::atomic<long> failures{0};
static const char *case_name = "(no case)";
static int case_slots = 0;

static void failed(const char *what, int line)
{
    if (failures++ < 50)
        printf("FAIL %s<%d> line %d: %s\n", case_name, case_slots, line, what);
}
#define CHECK(cond) do { if (!(cond)) failed(#cond, __LINE__); } while (0)

// ---- the fake runtime -------------------------------------------------------------------------------
namespace fake {
enum kind { GRAPH, EXEC, EVENT, KINDS };
enum call { CAPTURE_STREAM, BEGIN_CAPTURE, ENQUEUE, END_CAPTURE, INSTANTIATE, EVENT_CREATE, GRAPH_DESTROY,
            EXEC_DESTROY, EVENT_DESTROY, EVENT_QUERY, EVENT_RECORD, GET_DEVICE, GET_LAST_ERROR, CALLS };
constexpr int FAILURE_EXITS = 6;        // CAPTURE_STREAM .. EVENT_CREATE: the steps that make acquire() give up

struct handle {
    unsigned magic;
    long serial;        // (addresses are used again by the allocator: this is not)
    kind k;
    int device;
    // events
    bool recorded, ready, poisoned;
    hipStream_t stream;
    long records;
    // execs: replays a holder is still enqueuing, replays enqueued and not yet covered by a recorded
    // event, and the event that covers them
    int holders;
    bool awaiting_record;
    handle *guard;
};

static std::mutex mu;                   // the fake's own state (cases call it from outside the cache's lock)
static std::set<handle *> live;
static long created[KINDS], destroyed[KINDS], calls[CALLS], injected, serials;
static int fail_in[CALLS];              // n > 0: the n-th call from now fails
static bool sticky_not_ready;           // hipErrorNotReady is recorded as the thread's last error
static thread_local hipError_t last_error = hipSuccess;
static thread_local int device = 0;
static thread_local bool capturing = false;
static thread_local char stream_tag;    // its address is this thread's capture stream

static void problem(const char *what)
{
    failed(what, 0);
}

static long live_of(kind k) { return created[k] - destroyed[k]; }

static void reset()
{
    std::lock_guard<std::mutex> lock(mu);
    for (handle *h : live)
        delete h;
    live.clear();
    memset(created, 0, sizeof(created));
    memset(destroyed, 0, sizeof(destroyed));
    memset(calls, 0, sizeof(calls));
    memset(fail_in, 0, sizeof(fail_in));
    injected = 0;
    sticky_not_ready = false;
    last_error = hipSuccess;
    device = 0;
    capturing = false;
}

// (all of the following under `mu`)
static bool fails(call c)
{
    calls[c]++;
    if (fail_in[c] > 0 && --fail_in[c] == 0) {
        injected++;
        return true;
    }
    return false;
}

static hipError_t ret(hipError_t e)
{
    if (e != hipSuccess && (e != hipErrorNotReady || sticky_not_ready))
        last_error = e;
    return e;
}

static handle *make(kind k)
{
    handle *h = new handle();
    h->magic = 0xfa4e0000u + k;
    h->k = k;
    h->serial = ++serials;
    h->device = device;
    live.insert(h);
    created[k]++;
    return h;
}

// The live handle behind `p`, or null (and a failed check) for a null, dead or foreign one.
static handle *get(void *p, kind k, const char *what)
{
    handle *h = static_cast<handle *>(p);
    if (p == nullptr || !live.count(h)) {
        problem(what);
#ifdef HARNESS_ASAN
        if (p != nullptr)
            (void) *static_cast<volatile unsigned *>(p);    // the sanitizer's report names the two stacks
#endif
        return nullptr;
    }
    if (h->magic != 0xfa4e0000u + k) {
        problem("a handle of the wrong kind");
        return nullptr;
    }
    return h;
}

static hipError_t destroy(void *p, kind k, const char *what)
{
    handle *h = get(p, k, what);
    if (!h)
        return ret(hipErrorInvalidHandle);
    if (k == EXEC) {
        if (h->holders > 0 || h->awaiting_record)
            problem("an exec destroyed while a call holds it");
        else if (h->guard && live.count(h->guard) && h->guard->recorded && !h->guard->ready)
            problem("an exec destroyed while its replays are in flight");
    }
    live.erase(h);
    destroyed[k]++;
    h->magic = 0xdead;
    delete h;
    return hipSuccess;
}

// What a case does to the fake from outside the cache.
static void forget(void *p)             // (a cache that goes away takes what it owns with it)
{
    std::lock_guard<std::mutex> lock(mu);
    handle *h = static_cast<handle *>(p);
    if (live.erase(h)) {
        destroyed[h->k]++;
        delete h;
    }
}
static void arm(call c, int nth = 1) { std::lock_guard<std::mutex> lock(mu); fail_in[c] = nth; }
static bool is_live(void *p) { std::lock_guard<std::mutex> lock(mu); return live.count(static_cast<handle *>(p)) != 0; }
// the serial number of a live handle; 0 for anything else
static long serial(void *p)
{
    std::lock_guard<std::mutex> lock(mu);
    return live.count(static_cast<handle *>(p)) ? static_cast<handle *>(p)->serial : 0;
}
static void fire(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(mu);
    if (handle *h = get(e, EVENT, "fire: a dead event"))
        h->ready = true;
}
static void poison(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(mu);
    if (handle *h = get(e, EVENT, "poison: a dead event"))
        h->poisoned = true;
}
template <class RNG> static void fire_some(RNG &rng)
{
    std::lock_guard<std::mutex> lock(mu);
    for (handle *h : live)
        if (h->k == EVENT && h->recorded && rng() % 2)
            h->ready = true;
}
static handle event_state(hipEvent_t e)
{
    std::lock_guard<std::mutex> lock(mu);
    handle *h = get(e, EVENT, "event_state: a dead event");
    return h ? *h : handle();
}
// A holder of `exec` enqueues a replay of it (hipGraphLaunch), covered by `event` once recorded ...
static void launch(hipGraphExec_t exec, hipEvent_t event)
{
    std::lock_guard<std::mutex> lock(mu);
    handle *x = get(exec, EXEC, "launch: a dead exec");
    handle *e = get(event, EVENT, "launch: a dead event");
    if (x && e) {
        x->holders++;
        x->guard = e;
        e->guard = x;
    }
}
// ... and has enqueued its last one (what follows is the cache's release())
static void done(hipGraphExec_t exec)
{
    std::lock_guard<std::mutex> lock(mu);
    if (handle *x = get(exec, EXEC, "done: a dead exec")) {
        x->holders--;
        x->awaiting_record = true;
    }
}
}   // namespace fake

hipStream_t kimg_capture_stream()
{
    std::lock_guard<std::mutex> lock(fake::mu);
    if (fake::fails(fake::CAPTURE_STREAM))
        return nullptr;
    return reinterpret_cast<hipStream_t>(&fake::stream_tag);
}

extern "C" {
hipError_t hipStreamBeginCapture(hipStream_t stream, hipStreamCaptureMode mode)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    if (stream != reinterpret_cast<hipStream_t>(&fake::stream_tag))
        fake::problem("capture on a stream that is not the library's own");
    if (mode != hipStreamCaptureModeThreadLocal)
        fake::problem("capture mode is not thread-local");
    if (fake::capturing)
        fake::problem("begin capture on a capturing stream");
    if (fake::fails(fake::BEGIN_CAPTURE))
        return fake::ret(hipErrorStreamCaptureUnsupported);
    fake::capturing = true;
    return hipSuccess;
}

hipError_t hipStreamEndCapture(hipStream_t stream, hipGraph_t *graph)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    *graph = nullptr;
    if (!fake::capturing) {
        fake::problem("end capture without a capture");
        return fake::ret(hipErrorIllegalState);
    }
    fake::capturing = false;
    if (fake::fails(fake::END_CAPTURE))
        return fake::ret(hipErrorStreamCaptureInvalidated);
    *graph = reinterpret_cast<hipGraph_t>(fake::make(fake::GRAPH));
    return hipSuccess;
}

hipError_t hipGraphInstantiate(hipGraphExec_t *exec, hipGraph_t graph, hipGraphNode_t *, char *, size_t)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    if (!fake::get(graph, fake::GRAPH, "instantiate: a dead graph"))
        return fake::ret(hipErrorInvalidValue);
    if (fake::fails(fake::INSTANTIATE))
        return fake::ret(hipErrorOutOfMemory);
    *exec = reinterpret_cast<hipGraphExec_t>(fake::make(fake::EXEC));
    return hipSuccess;
}

hipError_t hipGraphDestroy(hipGraph_t graph)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    fake::calls[fake::GRAPH_DESTROY]++;
    return fake::destroy(graph, fake::GRAPH, "graph destroyed twice, or never made");
}

hipError_t hipGraphExecDestroy(hipGraphExec_t exec)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    fake::calls[fake::EXEC_DESTROY]++;
    return fake::destroy(exec, fake::EXEC, "exec destroyed twice, or never made");
}

hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned flags)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    if (flags != hipEventDisableTiming)
        fake::problem("an event with timing");
    if (fake::fails(fake::EVENT_CREATE))
        return fake::ret(hipErrorOutOfMemory);
    *event = reinterpret_cast<hipEvent_t>(fake::make(fake::EVENT));
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t event)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    fake::calls[fake::EVENT_DESTROY]++;
    return fake::destroy(event, fake::EVENT, "event destroyed twice, or never made");
}

hipError_t hipEventQuery(hipEvent_t event)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    fake::calls[fake::EVENT_QUERY]++;
    fake::handle *h = fake::get(event, fake::EVENT, "query of a dead event");
    if (!h || h->poisoned)
        return fake::ret(hipErrorInvalidHandle);
    // (an event that was never recorded counts as complete, as in the runtime)
    return fake::ret(!h->recorded || h->ready ? hipSuccess : hipErrorNotReady);
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    fake::calls[fake::EVENT_RECORD]++;
    fake::handle *h = fake::get(event, fake::EVENT, "record of a dead event");
    if (!h)
        return fake::ret(hipErrorInvalidHandle);
    if (h->device != fake::device)
        fake::problem("an event recorded on a stream of another device");
    h->recorded = true;
    h->ready = false;
    h->stream = stream;
    h->records++;
    if (h->guard && fake::live.count(h->guard))
        h->guard->awaiting_record = false;
    return hipSuccess;
}

hipError_t hipGetDevice(int *device)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    fake::calls[fake::GET_DEVICE]++;
    *device = fake::device;
    return hipSuccess;
}

hipError_t hipGetLastError(void)
{
    std::lock_guard<std::mutex> lock(fake::mu);
    fake::calls[fake::GET_LAST_ERROR]++;
    const hipError_t e = fake::last_error;
    fake::last_error = hipSuccess;
    return e;
}

hipError_t hipPeekAtLastError(void)
{
    return fake::last_error;
}
}   // extern "C"

// ---- a cache under test -----------------------------------------------------------------------------
struct args {
    char tag;           // (seven padding bytes follow)
    int64_t id;
    int n;              // (and four more here: the last byte of the struct is padding)
};
static_assert(sizeof(args) == 24, "the padding the cases rely on");

static args make_args(int64_t id)
{
    args a;
    memset(&a, 0, sizeof(a));
    a.tag = 'k';
    a.id = id;
    a.n = 7;
    return a;
}

static hipStream_t user_stream(int i)
{
    static char tags[16];
    return reinterpret_cast<hipStream_t>(&tags[i]);
}

template <int SLOTS> struct rig {
    using cache_t = kimg_graph_cache<args, SLOTS>;
    using entry = typename cache_t::entry;
    // `slots` is the cache's first member: a pointer to a standard-layout object is a pointer to it
    static_assert(std::is_standard_layout<cache_t>::value, "slots() reads the cache's first member");
    static_assert(sizeof(cache_t) >= SLOTS * sizeof(entry), "");

    cache_t *cache = new cache_t();     // value-initialised: zeroed, as an object with static storage is

    rig()
    {
        CHECK(fake::live.empty());
        fake::reset();
    }

    entry *slots() { return reinterpret_cast<entry *>(cache); }

    entry *acquire(const args &a)
    {
        entry *e = cache->acquire(a, [&](hipStream_t cs) {
            std::lock_guard<std::mutex> lock(fake::mu);
            if (!fake::capturing || cs != reinterpret_cast<hipStream_t>(&fake::stream_tag))
                fake::problem("launches outside a capture");
            if (fake::fails(fake::ENQUEUE)) {
                // (a launch failed: the runtime remembers it, and the capture is still open)
                fake::last_error = hipErrorLaunchFailure;
                return -(int) hipErrorLaunchFailure;
            }
            return 0; });
        CHECK(!fake::capturing);
        if (e) {
            CHECK(e >= slots() && e < slots() + SLOTS && e->valid && e->users >= 1);
            CHECK(memcmp(&e->args, &a, sizeof(a)) == 0);
            fake::launch(e->exec, e->last_use);
        }
        return e;
    }

    void release(entry *e, hipStream_t s)
    {
        fake::done(e->exec);
        cache->release(e, s);
    }

    // acquire + release + the event fires: an entry that may be evicted
    entry *idle(const args &a)
    {
        entry *e = acquire(a);
        if (e) {
            release(e, user_stream(0));
            fake::fire(e->last_use);
        }
        return e;
    }

    std::vector<char> snapshot()
    {
        const char *p = reinterpret_cast<const char *>(slots());
        return std::vector<char>(p, p + SLOTS * sizeof(entry));
    }

    int valid()
    {
        int n = 0;
        for (int i = 0; i < SLOTS; i++)
            n += slots()[i].valid;
        return n;
    }

    // what the cache owns, and nothing else, is alive
    void check_balance()
    {
        std::lock_guard<std::mutex> lock(fake::mu);
        CHECK(fake::live_of(fake::GRAPH) == 0);
        CHECK(fake::live_of(fake::EXEC) == valid());
        CHECK(fake::live_of(fake::EVENT) == valid());
    }

    ~rig()
    {
        check_balance();
        for (int i = 0; i < SLOTS; i++)
            if (slots()[i].valid) {
                CHECK(fake::is_live(slots()[i].exec) && fake::is_live(slots()[i].last_use));
                for (int j = 0; j < i; j++)
                    CHECK(!slots()[j].valid || (slots()[j].exec != slots()[i].exec
                                                && slots()[j].last_use != slots()[i].last_use));
            }
        for (int i = 0; i < SLOTS; i++)
            if (slots()[i].valid) {
                fake::forget(slots()[i].exec);
                fake::forget(slots()[i].last_use);
            }
        delete cache;
    }
};

static bool last_error_is(hipError_t want)
{
    return hipGetLastError() == want;
}

// ---- the cases --------------------------------------------------------------------------------------
template <int SLOTS> static void hit_and_miss()
{
    rig<SLOTS> r;
    const args a = make_args(1);
    auto *e1 = r.acquire(a);
    auto *e2 = r.acquire(a);
    CHECK(e1 != nullptr && e1 == e2);
    CHECK(fake::created[fake::EXEC] == 1 && fake::calls[fake::BEGIN_CAPTURE] == 1);
    CHECK(e1 && e1->users == 2);
    r.release(e1, user_stream(0));
    CHECK(e1->users == 1);
    r.release(e2, user_stream(0));
    CHECK(e1->users == 0);
    // one byte of a field, one byte of the inner padding, the last byte of the struct (padding too)
    long captures = 1;
    for (size_t byte : {size_t(8), size_t(1), sizeof(args) - 1}) {
        args b = a;
        reinterpret_cast<char *>(&b)[byte] ^= 1;
        auto *e = r.acquire(b);
        CHECK(e != nullptr && e != e1);
        CHECK(fake::created[fake::EXEC] == ++captures);
        if (e)
            r.release(e, user_stream(0));
    }
    auto *e3 = r.acquire(a);            // (still there)
    CHECK(e3 == e1 && fake::created[fake::EXEC] == captures);
    if (e3)
        r.release(e3, user_stream(0));
}

template <int SLOTS> static void fill_order()
{
    rig<SLOTS> r;
    std::set<void *> seen;
    for (int i = 0; i < SLOTS; i++) {
        // (everything stored so far could be evicted: an invalid slot is taken all the same)
        auto *e = r.idle(make_args(i));
        CHECK(e != nullptr && seen.insert(e).second);
        CHECK(fake::calls[fake::EXEC_DESTROY] == 0 && fake::calls[fake::EVENT_DESTROY] == 0);
        CHECK(fake::calls[fake::GRAPH_DESTROY] == i + 1 && fake::created[fake::GRAPH] == i + 1);
        CHECK(fake::calls[fake::EVENT_QUERY] == 0);
    }
    CHECK(r.valid() == SLOTS);
    CHECK(r.idle(make_args(SLOTS)) != nullptr);
    CHECK(fake::calls[fake::EXEC_DESTROY] == 1 && fake::calls[fake::EVENT_DESTROY] == 0);
}

template <int SLOTS> static void eviction_rule()
{
    for (int evictable : {SLOTS - 1, 1, -1}) {
        rig<SLOTS> r;
        std::vector<typename rig<SLOTS>::entry *> e(SLOTS);
        // even slots stay pinned, odd ones are released with an event that has not fired
        for (int i = 0; i < SLOTS; i++) {
            e[i] = r.acquire(make_args(i));
            if (e[i] && (i % 2 || i == evictable))
                r.release(e[i], user_stream(1));
        }
        if (evictable >= 0)
            fake::fire(e[evictable]->last_use);
        const auto before = r.snapshot();
        const long made = fake::created[fake::EXEC], events = fake::created[fake::EVENT];
        const long captures = fake::calls[fake::BEGIN_CAPTURE];
        const long old_exec = evictable >= 0 ? fake::serial(e[evictable]->exec) : 0;
        const long old_event = evictable >= 0 ? fake::serial(e[evictable]->last_use) : 0;
        auto *got = r.acquire(make_args(100));
        if (evictable < 0) {
            // every entry busy: null, nothing made, nothing destroyed, nothing changed
            CHECK(got == nullptr);
            CHECK(r.snapshot() == before);
            CHECK(fake::created[fake::EXEC] == made && fake::calls[fake::BEGIN_CAPTURE] == captures);
            CHECK(fake::calls[fake::EXEC_DESTROY] == 0 && fake::calls[fake::EVENT_DESTROY] == 0);
            CHECK(fake::live_of(fake::GRAPH) == 0);
        } else {
            CHECK(got == e[evictable]);
            CHECK(fake::calls[fake::EXEC_DESTROY] == 1 && got && fake::serial(got->exec) > old_exec);
            CHECK(fake::created[fake::EXEC] == made + 1);
            // the event is reused on the same device
            CHECK(fake::created[fake::EVENT] == events && fake::calls[fake::EVENT_DESTROY] == 0);
            CHECK(got && fake::serial(got->last_use) == old_event && got->users == 1 && !got->used);
            for (int i = 0; i < SLOTS; i++)
                if (i != evictable)
                    CHECK(memcmp(&before[i * sizeof(*got)], &r.slots()[i], sizeof(*got)) == 0);
        }
        for (int i = 0; i < SLOTS; i++)
            if (e[i] && !(i % 2 || i == evictable))
                r.release(e[i], user_stream(1));
        if (got)
            r.release(got, user_stream(1));
    }
}

template <int SLOTS> static void device_takeover()
{
    rig<SLOTS> r;
    for (int i = 0; i < SLOTS; i++)
        CHECK(r.idle(make_args(i)) != nullptr);
    for (int i = 0; i < SLOTS; i++)
        CHECK(r.slots()[i].device == 0);
    fake::device = 1;
    auto *e0 = r.acquire(make_args(100));       // (stays pinned)
    CHECK(e0 == &r.slots()[0]);
    // (the fake numbers its handles: the first 3 * SLOTS were the graphs, execs and events of the fill)
    CHECK(e0 && fake::serial(e0->exec) > 3 * SLOTS && fake::serial(e0->last_use) > 3 * SLOTS);
    CHECK(fake::calls[fake::EXEC_DESTROY] == 1 && fake::calls[fake::EVENT_DESTROY] == 1);
    CHECK(fake::created[fake::EVENT] == SLOTS + 1);
    CHECK(e0 && e0->device == 1 && e0->last_use != nullptr && fake::is_live(e0->last_use));
    CHECK(e0 && fake::event_state(e0->last_use).device == 1);
    // the next take-over, with the new event's creation failing
    const auto before = r.snapshot();
    const long execs = fake::created[fake::EXEC];
    fake::arm(fake::EVENT_CREATE);
    CHECK(r.acquire(make_args(101)) == nullptr);
    CHECK(fake::injected == 1);
    CHECK(!r.slots()[1].valid);
    CHECK(fake::calls[fake::EXEC_DESTROY] == 3 && fake::calls[fake::EVENT_DESTROY] == 2);
    CHECK(fake::created[fake::EXEC] == execs + 1 && fake::live_of(fake::EXEC) == SLOTS - 1);
    CHECK(last_error_is(hipSuccess));
    for (int i = 0; i < SLOTS; i++)
        if (i != 1)
            CHECK(memcmp(&before[i * sizeof(*e0)], &r.slots()[i], sizeof(*e0)) == 0);
    r.check_balance();
    // the slot can be used again
    auto *e1 = r.acquire(make_args(102));
    CHECK(e1 == &r.slots()[1] && e1->valid && e1->device == 1 && fake::is_live(e1->last_use));
    CHECK(fake::calls[fake::EXEC_DESTROY] == 3 && fake::calls[fake::EVENT_DESTROY] == 2);
    if (e1)
        r.release(e1, user_stream(0));
    if (e0)
        r.release(e0, user_stream(0));
}

template <int SLOTS> static void failure_exits()
{
    static const char *names[fake::FAILURE_EXITS] = {"no capture stream", "begin capture", "a launch in the capture",
                                                     "end capture", "instantiate", "event creation"};
    for (int full = 0; full < 2; full++)
        for (int step = 0; step < fake::FAILURE_EXITS; step++) {
            if (full && step == fake::EVENT_CREATE)
                continue;       // (an eviction on the same device creates no event: device_takeover has the other)
            rig<SLOTS> r;
            for (int i = 0; i < (full ? SLOTS : SLOTS - 1); i++)
                CHECK(r.idle(make_args(i)) != nullptr);
            const auto before = r.snapshot();
            const long graphs = fake::created[fake::GRAPH], ends = fake::calls[fake::END_CAPTURE];
            const long live_execs = fake::live_of(fake::EXEC), live_events = fake::live_of(fake::EVENT);
            fake::arm(fake::call(step));
            auto *e = r.acquire(make_args(100));
            if (e != nullptr || fake::injected != 1 || r.snapshot() != before)
                printf("(failure exit: %s, cache %s)\n", names[step], full ? "full" : "with a free slot");
            CHECK(e == nullptr);
            CHECK(fake::injected == 1);
            CHECK(r.snapshot() == before);
            CHECK(fake::live_of(fake::GRAPH) == 0);
            CHECK(fake::live_of(fake::EXEC) == live_execs && fake::live_of(fake::EVENT) == live_events);
            if (step == fake::ENQUEUE)
                // the capture is ended all the same, and its graph destroyed
                CHECK(fake::calls[fake::END_CAPTURE] == ends + 1 && fake::created[fake::GRAPH] == graphs + 1);
            // the failed call's error has been read: the plain launches that follow report their own
            CHECK(kimg_launch_status() == 0);
            // ... and the same arguments are cached by the next call
            e = r.acquire(make_args(100));
            CHECK(e != nullptr);
            if (e)
                r.release(e, user_stream(0));
        }
    // the converse: a call that succeeds leaves an error from before it for its owner to read
    rig<SLOTS> r;
    fake::last_error = hipErrorInvalidValue;
    auto *e = r.acquire(make_args(1));          // (captured)
    CHECK(e != nullptr && last_error_is(hipErrorInvalidValue));
    fake::last_error = hipErrorInvalidValue;
    auto *again = r.acquire(make_args(1));      // (found)
    CHECK(again == e && last_error_is(hipErrorInvalidValue));
    if (e)
        r.release(e, user_stream(0));
    if (again)
        r.release(again, user_stream(0));
}

template <int SLOTS> static void release_rule()
{
    rig<SLOTS> r;
    auto *e = r.acquire(make_args(0));
    CHECK(r.acquire(make_args(0)) == e);
    std::vector<typename rig<SLOTS>::entry *> others;
    for (int i = 1; i < SLOTS; i++)
        others.push_back(r.acquire(make_args(i)));      // (pinned)
    CHECK(e && !e->used && e->users == 2);
    r.release(e, user_stream(3));
    CHECK(e->used && e->users == 1);
    fake::handle ev = fake::event_state(e->last_use);
    CHECK(ev.recorded && !ev.ready && ev.stream == user_stream(3) && ev.records == 1);
    // its event fires, and the other user still holds it
    fake::fire(e->last_use);
    CHECK(r.acquire(make_args(100)) == nullptr);
    r.release(e, user_stream(4));
    ev = fake::event_state(e->last_use);
    CHECK(e->users == 0 && ev.stream == user_stream(4) && ev.records == 2 && !ev.ready);
    CHECK(r.acquire(make_args(100)) == nullptr);        // (the second record has not fired)
    fake::fire(e->last_use);
    auto *taken = r.acquire(make_args(100));
    CHECK(taken == e);
    if (taken)
        r.release(taken, user_stream(0));
    for (auto *o : others)
        if (o)
            r.release(o, user_stream(0));
}

// An event whose query fails with something other than "not ready" (an event of another device, on a
// runtime that minds): its slot can never be evicted.  The rest of the cache goes on working, the
// slot's own arguments still hit, and the failed queries leave no error behind.
template <int SLOTS> static void unqueryable_event()
{
    rig<SLOTS> r;
    auto *stuck = r.idle(make_args(0));
    CHECK(stuck != nullptr);
    if (!stuck)
        return;
    fake::poison(stuck->last_use);
    const long exec = fake::serial(stuck->exec);
    for (int i = 1; i < 3 * SLOTS; i++) {
        auto *e = r.idle(make_args(i));
        CHECK(e != nullptr && e != stuck);
        CHECK(kimg_launch_status() == 0);
    }
    CHECK(fake::calls[fake::EXEC_DESTROY] == 2 * SLOTS && fake::serial(stuck->exec) == exec);
    const long execs = fake::created[fake::EXEC];
    auto *e = r.acquire(make_args(0));
    CHECK(e == stuck && fake::created[fake::EXEC] == execs);
    if (e)
        r.release(e, user_stream(0));
}

// A runtime that records "not ready" as the thread's last error: what kimg_launch_status() reads after
// the two exits of acquire() that query events and do not go through give_up().
template <int SLOTS> static void not_ready_is_not_an_error()
{
    for (int stale = 0; stale < 2; stale++) {
        rig<SLOTS> r;
        fake::sticky_not_ready = true;
        std::vector<typename rig<SLOTS>::entry *> e(SLOTS);
        for (int i = 0; i < SLOTS; i++) {
            e[i] = r.acquire(make_args(i));
            if (e[i])
                r.release(e[i], user_stream(0));
        }
        // every entry busy
        if (stale)
            fake::last_error = hipErrorInvalidValue;
        const long queries = fake::calls[fake::EVENT_QUERY];
        CHECK(r.acquire(make_args(100)) == nullptr);
        CHECK(fake::calls[fake::EVENT_QUERY] == queries + SLOTS);
        CHECK(stale ? kimg_launch_status() != 0 : kimg_launch_status() == 0);
        // an eviction that passed over entries that were not ready
        fake::fire(e[SLOTS - 1]->last_use);
        if (stale)
            fake::last_error = hipErrorInvalidValue;
        auto *got = r.acquire(make_args(100));
        CHECK(got == e[SLOTS - 1]);
        CHECK(stale ? kimg_launch_status() != 0 : kimg_launch_status() == 0);
        if (got)
            r.release(got, user_stream(0));
    }
}

// ---- the model check ----------------------------------------------------------------------------------
// The rules restated on a plain map: which arguments are stored, who holds them, whether their event is
// pending.  Which evictable entry a new argument set takes is the cache's choice; the model checks that
// the one taken was evictable (and that an invalid slot, while there is one, comes first).
struct model_entry {
    int users;
    bool used, pending, unqueryable;
    int device;
    void *slot;
    bool evictable() const { return users == 0 && (!used || (!pending && !unqueryable)); }
};

template <int SLOTS> static void model_check()
{
    for (unsigned seed = 1; seed <= 2; seed++) {
        rig<SLOTS> r;
        using entry = typename rig<SLOTS>::entry;
        fake::sticky_not_ready = seed == 2;
        std::mt19937 rng(seed * 7919 + SLOTS);
        std::map<int64_t, model_entry> model;
        std::vector<std::pair<entry *, int64_t>> held;
        long captures = 0, hits = 0, nulls = 0, evictions = 0, unqueryable = 0;
        for (int step = 0; step < 20000 && failures == 0; step++) {
            unsigned op = rng() % 100;
            if (op < 50 && held.size() > SLOTS / 2 && rng() % 2)
                op = 50;        // (about half the entries pinned, most of the time)
            if (op < 50) {
                const int64_t id = rng() % (2 * SLOTS);
                const bool stale = rng() % 16 == 0;
                if (stale)
                    fake::last_error = hipErrorInvalidValue;
                const long injected = fake::injected, begun = fake::calls[fake::BEGIN_CAPTURE];
                const bool armed_event = fake::fail_in[fake::EVENT_CREATE] > 0;
                entry *e = r.acquire(make_args(id));
                const bool failed_step = fake::injected > injected;
                auto found = model.find(id);
                if (found != model.end()) {
                    CHECK(e == found->second.slot && !failed_step && fake::calls[fake::BEGIN_CAPTURE] == begun);
                    found->second.users++;
                    hits++;
                } else {
                    const bool free_slot = (int) model.size() < SLOTS;
                    bool candidate = free_slot;
                    for (auto &m : model)
                        candidate |= m.second.evictable();
                    if (!candidate) {
                        CHECK(e == nullptr && !failed_step && fake::calls[fake::BEGIN_CAPTURE] == begun);
                    } else {
                        CHECK((e == nullptr) == failed_step);
                        // the entry that was stored where the new one is, or whose slot became invalid
                        auto victim = model.end();
                        for (auto m = model.begin(); m != model.end(); ++m)
                            if ((e && m->second.slot == e) || (!e && !static_cast<entry *>(m->second.slot)->valid)) {
                                CHECK(victim == model.end());
                                victim = m;
                            }
                        if (victim != model.end()) {
                            CHECK(!free_slot && victim->second.evictable());
                            if (!e)     // (only a take-over whose new event could not be made ends like this)
                                CHECK(armed_event && victim->second.device != fake::device);
                            unqueryable -= victim->second.unqueryable;
                            model.erase(victim);
                            evictions++;
                        } else if (e)
                            CHECK(free_slot);
                        if (e) {
                            CHECK(e->device == fake::device && e->users == 1 && !e->used);
                            model[id] = model_entry{1, false, false, false, fake::device, e};
                            captures++;
                        }
                    }
                }
                if (e)
                    held.push_back({e, id});
                else
                    nulls++;
                // an error from before the call is still there after a call that made or found a graph;
                // otherwise nothing is left behind
                if (stale)
                    CHECK((hipGetLastError() != hipSuccess) || !e);
                else
                    CHECK(last_error_is(hipSuccess));
            } else if (op < 78) {
                if (held.empty())
                    continue;
                const size_t k = rng() % held.size();
                entry *e = held[k].first;
                model_entry &m = model[held[k].second];
                held.erase(held.begin() + k);
                // (a call releases on the device it acquired on)
                const int device = fake::device;
                fake::device = m.device;
                hipStream_t s = user_stream(rng() % 8);
                r.release(e, s);
                fake::device = device;
                m.users--;
                m.used = m.pending = true;
                CHECK(e->used && e->users == m.users);
                const fake::handle ev = fake::event_state(e->last_use);
                CHECK(ev.recorded && !ev.ready && ev.stream == s);
            } else if (op < 90) {
                for (auto &m : model)
                    if (m.second.pending && rng() % 3 == 0) {
                        fake::fire(static_cast<entry *>(m.second.slot)->last_use);
                        m.second.pending = false;
                    }
            } else if (op < 94) {
                fake::device = rng() % 3;
            } else if (op < 99) {
                bool armed = false;
                for (int c = 0; c < fake::FAILURE_EXITS; c++)
                    armed |= fake::fail_in[c] > 0;
                if (!armed)
                    fake::arm(fake::call(rng() % fake::FAILURE_EXITS));
            } else if (!model.empty() && unqueryable < SLOTS / 2) {
                auto m = model.begin();
                std::advance(m, rng() % model.size());
                if (!m->second.unqueryable) {
                    fake::poison(static_cast<entry *>(m->second.slot)->last_use);
                    m->second.unqueryable = true;
                    unqueryable++;
                }
            }
            // what is alive is what the model says is stored
            CHECK(r.valid() == (int) model.size());
            r.check_balance();
            CHECK(fake::created[fake::EXEC] - fake::destroyed[fake::EXEC] == (long) model.size());
            long users = 0;
            for (int i = 0; i < SLOTS; i++)
                users += r.slots()[i].valid ? r.slots()[i].users : 0;
            CHECK(users == (long) held.size());
        }
        // (the walk went everywhere)
        CHECK(captures > 100 && hits > 100 && nulls > 100 && evictions > 100 && fake::injected > 100);
        for (auto &h : held) {
            fake::device = model[h.second].device;
            r.release(h.first, user_stream(0));
        }
    }
}

// ---- threads --------------------------------------------------------------------------------------------
template <int SLOTS> static void threads()
{
    rig<SLOTS> r;
    constexpr int THREADS = 8, PAIRS = 3000;
    std::atomic<long> got{0}, fell_back{0};
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; t++)
        pool.emplace_back([&, t] {
            std::mt19937 rng(1000 + t);
            for (int i = 0; i < PAIRS; i++) {
                const args a = make_args(rng() % (2 * SLOTS));
                auto *e = r.cache->acquire(a, [](hipStream_t) { return 0; });
                if (e) {
                    // outside the lock: the entry is pinned, and it is the one asked for
                    CHECK(memcmp(&e->args, &a, sizeof(a)) == 0);
                    fake::launch(e->exec, e->last_use);
                    if (rng() % 4 == 0)
                        std::this_thread::yield();
                    CHECK(memcmp(&e->args, &a, sizeof(a)) == 0);
                    r.release(e, user_stream(t));
                    got++;
                } else
                    fell_back++;
                if (rng() % 2)
                    fake::fire_some(rng);
            }
        });
    for (auto &th : pool)
        th.join();
    CHECK(got + fell_back == THREADS * PAIRS && got > THREADS * PAIRS / 4);
    for (int i = 0; i < SLOTS; i++)
        CHECK(r.slots()[i].valid && r.slots()[i].users == 0);
    CHECK(fake::calls[fake::EXEC_DESTROY] > 0);         // (entries were evicted)
    CHECK(fake::created[fake::EXEC] < got);             // (and found again)
    r.check_balance();
}

// ---- main -------------------------------------------------------------------------------------------------
template <int SLOTS> static void run(const char *name, void (*fn)(), const char *only)
{
    if (strcmp(only, "all") != 0 && strcmp(only, name) != 0)
        return;
    case_name = name;
    case_slots = SLOTS;
    const long before = failures;
    fake::reset();
    fn();
    {
        std::lock_guard<std::mutex> lock(fake::mu);
        CHECK(fake::live.empty());      // (the rig's cache is gone: what is left has leaked)
    }
    fake::reset();
    printf("%s %s<%d>\n", failures == before ? "ok" : "FAILED", name, SLOTS);
}

#define RUN(name) do { run<4>(#name, &name<4>, only); run<32>(#name, &name<32>, only); } while (0)

int main(int argc, char **argv)
{
    const char *only = argc > 1 ? argv[1] : "all";
    setvbuf(stdout, nullptr, _IOLBF, 0);
    RUN(hit_and_miss);
    RUN(fill_order);
    RUN(eviction_rule);
    RUN(device_takeover);
    RUN(failure_exits);
    RUN(release_rule);
    RUN(unqueryable_event);
    RUN(not_ready_is_not_an_error);
    RUN(model_check);
    RUN(threads);
    if (case_slots == 0) {
        printf("no such case: %s\n", only);
        return 2;
    }
    printf("%ld failed checks\n", (long) failures);
    return failures ? 1 : 0;
}
