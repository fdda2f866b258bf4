// What the translation units of the device gunzip share: the driver (ss_ginflate.hip), its process-wide device resources
// (ss_gz_scratch.hip) and range mode's chain between ranks (ss_gz_range.hip).  Not part of the C ABI; what the rest of the
// library calls is in ss_common.h.
#pragma once
#include "ss_common.h"

namespace ss {

constexpr uint32_t WSIZE = 32768;         // deflate's window: what a match may reach back

// ---- ss_gz_scratch.hip ----------------------------------------------------------------------------------------------------------
// Scratch of one call, kept for the next one: the per-segment symbol streams, window maps and chunk arrays.  (Allocating
// and freeing tens of GB per file is what this replaces: on this platform a large hipMalloc that follows a large hipFree
// can take 1.6 s -- scripts/archive/dev/t_bigalloc.py -- and a 1 GB .gz needed 28 GB of symbols in one piece.)  At most two are
// kept (the two mates of a pair are inflated concurrently), ~4.5 GB each, until the process ends.
struct Arena {
    uint64_t cap_chunks = 0, sym_elems = 0;
    uint16_t *sym = nullptr, *map[2] = {nullptr, nullptr};
    uint64_t *meta = nullptr;
    int *status = nullptr;
    uint8_t *win = nullptr, *gwin = nullptr, *prev = nullptr;
    uint32_t *todo = nullptr;
    uint8_t *text = nullptr;              // the text of the call that holds the arena (lent to the caller until gpu_gunzip_done)
    uint64_t text_cap = 0;
    void *late_free[4] = {nullptr, nullptr, nullptr, nullptr};      // the call's stage and lists: given back when the text is (the
                                                                     // frees took ~1 ms beside another thread's allocations, in front of the caller's work)
};
// The scratch of a call: an arena of at least cap_chunks chunks and sym_elems symbols whose text buffer holds text_cap bytes.
// `a`: one the call holds already, or null -- then a waiting one that needs no allocation, or, if the device has the memory
// (`beside`: what the call allocates apart from it), a new one.  null: *why says what was missing.
struct Why { const char *what = nullptr; long long arg = 0; };
Arena *acquire_scratch(Arena *a, uint64_t cap_chunks, uint64_t sym_elems, uint64_t text_cap, uint64_t beside, Why *why);
void arena_put(Arena *a);
bool pin_waiting();                       // a set of pinned upload buffers is waiting: the upload costs no allocation
// `ready(bytes)`: called (serialised, from the upload threads) whenever the PREFIX of the image that has arrived on the device
// has grown -- the caller starts work on it while the rest is still on its way.
bool upload_file(int fd, uint64_t n, uint8_t *d_in, const std::function<void(uint64_t)> &ready = nullptr);

// ---- ss_gz_range.hip (the chain is described there) -----------------------------------------------------------------------------
constexpr uint32_t CARRY_MAX = 65536;
struct ChainMsg {
    int32_t status;
    uint32_t crc;
    uint64_t len, nl, end_bit;
    uint32_t carry_len, pad;
    uint8_t window[WSIZE];
    uint8_t carry[CARRY_MAX];
};
struct RangeRun {
    uint32_t rank = 0, world = 1, slice_chunks = 0, n_slices = 0;
    uint64_t slice_bytes = 0;             // ss_gz_set_range's (0: by the file's size)
    ss_gz_chain_fn fn = nullptr;
    void *user = nullptr;
    std::vector<uint32_t> mine;           // my slices, ascending
    size_t duty = 0;                      // mine[duty]: the first slice whose part in the chain is not finished
    bool received = false;                // ... and whether its message has come in
    bool failed = false;                  // a callback failed: this rank declines, status -1 still goes down the chain
    bool broken = false;                  // a SEND failed: no more chain traffic
    bool inject_decline = false;          // test hook
    ChainMsg msg;                         // the last message received / the one being sent
    std::vector<GzPiece> *pieces = nullptr;
    uint64_t ticket = 0;                  // this file's place in the order in which the files of a load use the chain
    bool recv_for(uint32_t s);
    bool send_from(uint32_t s);
    void abort_chain();                   // whatever is left of this rank's part in the chain, as a bystander: receive, pass on that it went wrong
};

// ---- ss_ginflate.hip: one call of the driver; rr: the call inflates this rank's slices only (gpu_gunzip_range) -----------------------
bool gpu_gunzip_impl(const uint8_t *in, uint64_t in_n, char **text_dev, uint64_t *len, void **lease, int fd, RangeRun *rr);

}  // namespace ss
