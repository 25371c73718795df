// Internal declarations shared by the sharding protocol (shard.cpp), the RCCL communicator (rccl_comm.cpp), the C ABI
// (goicp_api.cpp) and the sanitizer driver (host_selftest.cpp).
#pragma once
#include <cstdint>

#include "../../include/goicp_mi355.h"

namespace goicp {

// first member of the context of every communicator the library makes (thread, RCCL): lets goicp_comm_set_timeout_ms
// find the deadline without knowing the kind
struct CommHeader { uint32_t magic; int32_t timeout_ms; };
constexpr uint32_t kCommMagic = 0x43494f47u;     // "GOIC"

int comm_default_timeout_ms();                   // GOICP_COMM_TIMEOUT_MS, else 60 000
int comm_set_timeout_ms(goicp_comm_ops* comm, int ms);
// A communicator of the library is recognised by its all-reduce FUNCTION (registered here by the kind that owns it), never by
// peeking into ctx: the ABI lets a caller bring its own communicator, whose ctx may be anything -- or nothing readable.
using CommAllreduceFn = int (*)(void*, uint64_t*, size_t);
// a kind's native element-wise SUM of n 64-bit words (wrapping mod 2^64), in place, blocking, under the same deadline
using CommSumFn = int (*)(void*, int64_t*, size_t);
void comm_register_library_kind(CommAllreduceFn fn, CommSumFn sum = nullptr);
bool comm_is_library_kind(const goicp_comm_ops* comm);
// goicp_comm_allreduce_sum_i64: the kind's native sum when the table is one of the library's, else `world` broadcasts of the n words
// (one from every rank) added up on every rank -- the same totals everywhere, since addition mod 2^64 is associative and commutative
int comm_allreduce_sum_i64(const goicp_comm_ops* comm, int64_t* words, size_t n);

// goicp_register_sharded_collective_icp: the engine side of the collective refinement, beside the public callback table
struct ShardIcpHooks {
	int (*unrefined)(void* ctx, int32_t* flag);      // 1: this rank's best pose is an upper bound ICP has not refined yet
	// every rank, together: collective ICP from pose (R|t, 12 floats), then the DT re-score; the rank's best pose counts as refined after it
	int (*refine)(void* ctx, const float pose[12], float* sse, float R[9], float t[3]);
};
// icp != nullptr: the winner's broadcast pose carries its unrefined flag, and an unrefined winner is refined collectively on every rank
// right after the exchange and offered (bulk-synchronous only: stale_exchange = 1 is GOICP_ERR_INVALID)
int run_sharded(const goicp_shard_engine_ops* eng, const goicp_comm_ops* comm, const goicp_shard_options* opt, goicp_shard_stats* stats,
                const ShardIcpHooks* icp = nullptr);
int thread_comm_create(int world, goicp_comm_ops* out);
void thread_comm_destroy(goicp_comm_ops* comm);

int rccl_unique_id(char id128[GOICP_RCCL_ID_BYTES]);
int rccl_comm_create(const char id128[GOICP_RCCL_ID_BYTES], int32_t rank, int32_t world, int32_t device, goicp_comm_ops* out);
int rccl_comm_wrap(void* nccl_comm, int32_t rank, int32_t world, int32_t device, goicp_comm_ops* out);
int rccl_comm_destroy(goicp_comm_ops* comm);
int rccl_comm_init_all(int world, void** comms);
void rccl_comm_destroy_raw(void* comm);

}  // namespace goicp
