// hipGraphs of a fixed run of launches, cached per argument set (clean.hip, clean_multi.hip): the
// CLEAN loops are launch-bound, and replaying a captured graph costs far less host time than the
// launches it holds.
#pragma once
#include "kimg_common.h"
#include <string.h>
#include <mutex>

// ARGS: a plain struct that holds every kernel argument of the run, compared byte by byte (callers
// memset it before they fill it: padding bytes take part).  One object per kind of run, with static
// storage (its slots start out zeroed).
template <class ARGS, int SLOTS>
class kimg_graph_cache {
public:
    struct entry {
        bool valid;
        int users;              // calls that hold `exec` and have not finished enqueuing its replays
        ARGS args;
        hipGraphExec_t exec;
        hipEvent_t last_use;    // recorded after the last replay enqueued by a finished call
        bool used;
        int device;             // the device `last_use` (and the graph) belongs to
    };

    // The cached graph for `a`, or one newly captured from what `enqueue_all(capture_stream)` launches
    // (0, or the code of the launch that failed); the entry stays pinned until release().  An entry is
    // only evicted when no call is using it and the replays enqueued from it have completed (its
    // event has fired), so a graph is never destroyed while it is in flight.  (An event whose query
    // fails with anything but "not ready" counts as not fired: its entry stays, and is still found.)
    // Null: every entry is busy, or the graph could not be made; the caller enqueues plain launches.
    template <class F> entry *acquire(const ARGS &a, F &&enqueue_all)
    {
        std::lock_guard<std::mutex> lock(mutex);
        for (int i = 0; i < SLOTS; i++)
            if (slots[i].valid && memcmp(&slots[i].args, &a, sizeof(a)) == 0) {
                slots[i].users++;
                return &slots[i];
            }
        entry *slot = nullptr;
        for (int i = 0; i < SLOTS && !slot; i++)
            if (!slots[i].valid)
                slot = &slots[i];
        if (!slot) {
            // (a query that answers "not ready", or fails, may stay behind as the thread's last error,
            // depending on the runtime; the caller's kimg_launch_status() would take it for a failed
            // launch.  It is read here -- unless an error from before this call is waiting, which is
            // not this call's to swallow)
            const bool clean = hipPeekAtLastError() == hipSuccess;
            for (int i = 0; i < SLOTS && !slot; i++)
                if (slots[i].users == 0
                    && (!slots[i].used || hipEventQuery(slots[i].last_use) == hipSuccess))
                    slot = &slots[i];
            if (clean)
                (void) hipGetLastError();
        }
        if (!slot)
            return nullptr;
        hipGraph_t graph = nullptr;
        // (captured on the library's own stream of this thread, launched on the caller's: see
        // kimg_capture_stream)
        hipStream_t cs = kimg_capture_stream();
        if (cs == nullptr || hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal) != hipSuccess)
            return give_up();
        const int rc = enqueue_all(cs);
        const hipError_t ended = hipStreamEndCapture(cs, &graph);
        if (ended != hipSuccess || rc != 0) {
            if (ended == hipSuccess && graph != nullptr)
                (void) hipGraphDestroy(graph);      // (a launch failed during the capture)
            return give_up();
        }
        hipGraphExec_t exec = nullptr;
        const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void) hipGraphDestroy(graph);
        if (e != hipSuccess)
            return give_up();
        // (imagers on several devices may share this process: an event is recorded on streams of the
        // device it was created on, so a slot taken over from another device gets a new one)
        int device = 0;
        (void) hipGetDevice(&device);
        if (slot->valid) {
            (void) hipGraphExecDestroy(slot->exec);
            if (slot->device != device) {
                (void) hipEventDestroy(slot->last_use);
                slot->valid = false;
            }
        }
        if (!slot->valid && hipEventCreateWithFlags(&slot->last_use, hipEventDisableTiming) != hipSuccess) {
            (void) hipGraphExecDestroy(exec);
            return give_up();
        }
        slot->device = device;
        slot->valid = true;
        slot->used = false;
        slot->users = 1;
        slot->args = a;
        slot->exec = exec;
        return slot;
    }

    // The call has enqueued its last replay of `e` on `s`.
    void release(entry *e, hipStream_t s)
    {
        std::lock_guard<std::mutex> lock(mutex);
        (void) hipEventRecord(e->last_use, s);
        e->used = true;
        e->users--;
    }

private:
    // A HIP call failed and the caller goes on with plain launches, which it checks with
    // kimg_launch_status(): the runtime keeps a thread's last error until somebody reads it, later
    // successful calls do not clear it, so it is read here -- or the caller's good launches would
    // report the failure of a capture they took no part in.
    static entry *give_up()
    {
        (void) hipGetLastError();
        return nullptr;
    }

    entry slots[SLOTS];
    std::mutex mutex;           // channels imaged concurrently share the cache
};
