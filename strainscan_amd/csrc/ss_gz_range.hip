// ss_gz_range.hip -- several ranks share ONE gzip member (ss_gz_set_range): the chain of messages between them.  The slices
// themselves are inflated by the driver (ss_ginflate.hip: gpu_gunzip_impl with a RangeRun).
// The deflate data is cut into slices of `slice_chunks` search chunks; slice s belongs to rank s mod world.  A rank looks
// for block starts in its slices only, inflates their chunks to symbols -- the expensive part, all ranks at once -- and
// then needs what lies in front of each slice: the last 32 KB of the text before it.  That comes from the owner of the
// slice before, down a CHAIN of small messages (the caller's callback: point-to-point send / receive between ranks):
//     window     the 32 KB in front of the next slice
//     end_bit    where this slice's last chunk ended: the next slice's first chunk must start exactly there
//     nl         newlines so far: the next rank knows which of the four FASTQ lines its text starts in
//     carry      the bytes behind the last complete record (its rest is in the next slice)
//     crc, len   CRC-32 and length of the text so far (the owner of the last slice checks them against the trailer)
//     status     < 0: somebody declined -- passed on to the end of the chain, everybody declines
// A rank that fails at any point still takes part in the chain for all its slices (receives, passes the bad news on), so
// nobody waits for a message that never comes.  Several members (lanes joined with cat) are followed inside the slices as in
// the whole-file path -- a member that ends in a slice is checked against its trailer by the slice's owner, crc / len
// always describe the member that is open at the cut.  bgzip: a slice's chunks are the members that begin in its byte range
// (no search, no window needed); the chain carries the newline count and the straddling record all the same.
// (ChainMsg and RangeRun: ss_ginflate.h -- the driver fills and reads the message.)
#include "ss_ginflate.h"

#include <condition_variable>
#include <mutex>

namespace ss {

// the order in which the files of a load use the chain (ss_common.h: gz_range_ticket)
static std::mutex g_turn_mu;
static std::condition_variable g_turn_cv;
static uint64_t g_turn_issued = 0, g_turn_serving = 0;
uint64_t gz_range_ticket()
{
    std::lock_guard<std::mutex> g(g_turn_mu);
    return g_turn_issued++;
}
static void gz_range_wait(uint64_t ticket)                   // (returns at once for the holder of the turn and for tickets already passed)
{
    std::unique_lock<std::mutex> g(g_turn_mu);
    g_turn_cv.wait(g, [&] { return g_turn_serving >= ticket; });
}
void gz_range_pass(uint64_t ticket)
{
    std::unique_lock<std::mutex> g(g_turn_mu);
    g_turn_cv.wait(g, [&] { return g_turn_serving >= ticket; });
    if (g_turn_serving == ticket) { g_turn_serving++; g_turn_cv.notify_all(); }
}

// A failed callback (the caller's point-to-point call raised, or its bounded wait ran out: dist._gz_chain) does not end
// this rank's part: nothing more is RECEIVED (the outcome is known: declined), but status -1 still goes down the chain
// for every slice of this rank, so that the ranks behind it learn it at once instead of each waiting for its own
// deadline; only a failed SEND ends the traffic (the peer is gone).
bool RangeRun::recv_for(uint32_t s)
{
    if (s == 0) return !failed;
    if (failed) return false;
    gz_range_wait(ticket);
    if (fn(&msg, sizeof(ChainMsg), (int)s, 0, user) != 0) { failed = true; msg.status = -1; msg.carry_len = 0; return false; }
    received = true;
    return true;
}
bool RangeRun::send_from(uint32_t s)
{
    if (s + 1 >= n_slices) return !failed;
    if (broken) return false;
    if (failed) { msg.status = -1; msg.carry_len = 0; }
    gz_range_wait(ticket);
    if (fn(&msg, sizeof(ChainMsg), (int)s, 1, user) != 0) { broken = true; failed = true; return false; }
    return !failed;
}
void RangeRun::abort_chain()
{
    for (; duty < mine.size() && !broken; duty++) {
        const uint32_t s = mine[duty];
        if (s > 0 && !received) recv_for(s);
        msg.status = -1;
        msg.carry_len = 0;
        send_from(s);
        received = false;
    }
}

static std::mutex g_range_mu;            // (guards g_range)
static struct { int rank = 0, world = 1; uint64_t slice_bytes = 0; ss_gz_chain_fn fn = nullptr; void *user = nullptr; } g_range;

bool gz_range_active() { return g_range.world > 1 && g_range.fn != nullptr; }

std::atomic<long long> g_hook_skip_chain{0};      // ss_test_hook 3: nothing in the environment can switch it on

// This rank's slices of the file: *text_dev holds their texts back to back, `pieces` says where each lies, what came down
// the chain in front of it (the bytes of a record that began in the slice before) and where its last complete record
// ends.  false: declined (the chain has been served all the same).
bool gpu_gunzip_range(const uint8_t *in, uint64_t in_n, char **text_dev, void **lease, int fd, std::vector<GzPiece> *pieces, uint64_t ticket, bool decline)
{
    RangeRun rr;
    {
        std::lock_guard<std::mutex> one(g_range_mu);
        if (!gz_range_active()) return false;
        rr.rank = (uint32_t)g_range.rank; rr.world = (uint32_t)g_range.world; rr.fn = g_range.fn; rr.user = g_range.user;
        rr.slice_bytes = g_range.slice_bytes;
    }
    if (g_hook_skip_chain.load()) return false;               // test hook: a rank that leaves WITHOUT serving the chain (the peers' bounded wait)
    rr.ticket = ticket;
    rr.pieces = pieces;
    rr.inject_decline = decline;
    uint64_t n = 0;
    const bool ok = gpu_gunzip_impl(in, in_n, text_dev, &n, lease, fd, &rr);
    gz_range_pass(ticket);                                    // (this file's chain traffic is over, whatever came of it)
    return ok;
}

}  // namespace ss

extern "C" int ss_gz_set_range(int rank, int world, uint64_t slice_bytes, ss_gz_chain_fn chain, void *user)
{
    if (world < 1 || rank < 0 || rank >= world) return SS_EINVAL;
    std::lock_guard<std::mutex> one(ss::g_range_mu);
    ss::g_range.rank = rank; ss::g_range.world = world; ss::g_range.slice_bytes = slice_bytes; ss::g_range.fn = chain; ss::g_range.user = user;
    return SS_OK;
}
