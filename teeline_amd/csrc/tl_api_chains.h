// tl_api_chains.h — what the calls over seeded chains share on the host (internal to libteeline_gpu): the checks of the common
// arguments, the instance with its full matrix, the per-CU chain count of a plan, the download of the results and the best
// chain.  tl_api_sa.hip, tl_api_tabu.hip and tl_api_ga.hip include it; each keeps its own option checks, workspace and launches.
// tl_api_swarm.h includes it too and builds the one host path of the population solvers (ant colony, particle swarm, cuckoo search,
// flower pollination, gravitational search) out of these pieces.
#pragma once
#include "tl_api_common.h"

namespace tlapi {

// tl_api_onetree.hip: nullptr where every distance of the instance is finite and >= +0.0, else what is wrong (also tl_api_alpha.hip's rule)
const char *one_tree_bad_input(const float *xy, const float *dm_packed, uint32_t n);

// The first checks of a call over `count` chains (noun "chain") or runs ("run") numbered from `first`.  count == 0 passes: the
// caller returns TL_OK at once.  init_count: 0 (city order), 1 (one start tour) or count.
inline int check_chain_call(tl_ctx *c, const char *who, const float *xy, const float *dm_packed, uint32_t count, const uint32_t *out_pos,
                            const uint32_t *init_pos, uint32_t init_count, uint32_t first, const char *noun)
{
    if (!c || (!xy && !dm_packed)) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (count == 0) return TL_OK;
    if (!out_pos || (init_count && !init_pos)) return fail(c, TL_ERR_BADARG, "%s: NULL argument", who);
    if (init_count != 0u && init_count != 1u && init_count != count)
        return fail(c, TL_ERR_BADARG, "%s: init_count is %u: 0 (city order), 1 (one start tour) or count (%u)", who, init_count, count);
    if ((uint64_t)first + count > 0x100000000ull) return fail(c, TL_ERR_BADARG, "%s: %s ids beyond 2^32 - 1", who, noun);
    return TL_OK;
}

// The instance onto the device (upload_input) and, where it is a matrix, its full n x n form into c->dmfull: then *d_full is set
// and *d_xy cleared.  The context's event pair is no longer valid from here on.
inline int upload_instance_full(tl_ctx *c, const float *xy, const float *dm_packed, uint32_t n, const float2 **d_xy, const float **d_full)
{
    int rc;
    const float *d_dm = nullptr;
    if ((rc = upload_input(c, xy, dm_packed, n, d_xy, &d_dm))) return rc;
    c->ev_valid = false;
    if (d_dm) {
        if ((rc = ws_order(c, c->stream))) return rc;  // dmfull may still be read by a batch this context enqueued on another stream
        if ((rc = ensure(c, c->dmfull, up256((size_t)n * n * 4)))) return rc;
        HIPCHK(c, tl::launch_dm_expand_full(d_dm, n, (float *)c->dmfull.p, c->stream));
        *d_full = (const float *)c->dmfull.p;
        *d_xy = nullptr;
    }
    return TL_OK;
}

// chains a CU holds at once: as many as its LDS and its 32 wave slots allow
inline uint64_t chains_per_cu(int lds_bytes, size_t lds_per_chain, int threads)
{
    const uint64_t per_cu = (uint64_t)lds_bytes / lds_per_chain;
    return per_cu > 2048u / (uint32_t)threads ? 2048u / (uint32_t)threads : per_cu;
}

// The per-chain records (rec_words words each, c->misc), costs and tours of a finished call, enqueued on the context's stream: the
// caller adds the copies of its own and synchronises.
inline int download_chains(tl_ctx *c, uint32_t count, uint32_t n, uint32_t rec_words, uint32_t *out_pos, std::vector<uint32_t> &run, std::vector<float> &costs)
{
    run.resize((size_t)count * rec_words);
    costs.resize(count);
    HIPCHK(c, hipMemcpyAsync(run.data(), c->misc.p, (size_t)count * rec_words * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(costs.data(), c->out_cost.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_pos, c->out_pos.p, (size_t)count * n * 4, hipMemcpyDeviceToHost, c->stream));
    return TL_OK;
}

// the chain of the lowest cost, then the lowest index
inline uint32_t best_chain(const std::vector<float> &costs, uint32_t count)
{
    uint32_t best = 0;
    uint64_t best_key = ~0ull;
    for (uint32_t r = 0; r < count; ++r) {
        const uint64_t k = tl_pack_cost_key(costs[r], r);
        if (k < best_key) {
            best_key = k;
            best = r;
        }
    }
    return best;
}

}  // namespace tlapi
