// ps_fwd.cpp — the chunk loop of candidate-sequence alignments: every event of an AlignData aligned forward-only to a sequence that is
// not its own (FindMutations' seeds, the variants of ps_score_sequences), for any number of such units, in as many launch chains as
// this runtime's share of the device allows.  What the two callers differ in — how ref_align of the jobs gets onto the device, what is
// read after the fills — they hand in as callbacks (ps_host.h).
#include <algorithm>

#include "ps_host.h"

namespace ps {

// Where the chunk that starts at unit q0 ends: as many units as the matrix budget `cap` holds (typical anti-diagonal footprint ~ half
// the band; p_seen: the widest one a chunk of this call turned out to need), at most `limit` of them, always at least one
// (greedy_cut, ps_plan.h)
static size_t fwd_chunk_end(const std::vector<FwdUnit>& units, size_t q0, double cap, int p_seen, size_t limit) {
    return greedy_cut(q0, units.size(), cap, limit, [&](size_t q) {
        const Align* a = units[q].a;
        const int C = (int)units[q].states->size();
        // slots per anti-diagonal as realign will probably size them (the first chunk finds out and is cut again if not)
        const int P = std::max(p_seen, guess_slots(a));
        double add = 0;
        for (int e = 0; e < a->E; e++)
            add += sweep_enabled() && sweep_guess_k(a->par.realign_width) ? fwd_job_bytes(a, a->n[e], C)
                                                                          : matrix_bytes((int64_t)a->n[e] + (int64_t)C + 1, P, 1);
        return add;
    });
}

int fwd_chunks(Runtime* rt, const std::vector<FwdUnit>& units, const char* what, const FwdStep& place, const FwdStep& collect,
               int* nchunks, Tick* tk) {
    const double cap = device_share_bytes();   // the DP-matrix bytes of one chunk: this runtime's share of the device (ps_mem.cpp)
    size_t q0 = 0;
    int p_seen = 0;              // widest anti-diagonal footprint (in slots) a chunk of this call turned out to need
    size_t limit = (size_t)-1;   // units per chunk after a chunk had to be cut again
    while (q0 < units.size()) {
        FwdChunk c;
        c.q0 = q0;
        c.q1 = fwd_chunk_end(units, q0, cap, p_seen, limit);
        const size_t n = c.q1 - c.q0;
        const size_t stage_mark = rt->stage.mark();
        c.roff.assign(n + 1, 0);
        for (size_t q = c.q0; q < c.q1; q++) {
            c.roff[q - q0 + 1] = c.roff[q - q0] + (size_t)units[q].a->ntot;
            c.njobs += units[q].a->E;
        }
        c.nref = c.roff[n];
        DBuf& rb = rt->buf("seed_refs");
        PS_TRY(rb.ensure((size_t)3 * std::max<size_t>(c.nref, 1) * sizeof(double)));
        c.d_ra = rb.as<double>();
        c.d_rl = c.d_ra + c.nref;
        c.d_ri = c.d_rl + c.nref;
        PS_TRY(place(c));
        DBuf& ob = rt->buf("seed_out");
        PS_TRY(ob.ensure(c.njobs * sizeof(JobOut)));   // (before the out pointers are taken: ensure() may move the buffer)
        PS_HIP(hipMemsetAsync(ob.p, 0, c.njobs * sizeof(JobOut), rt->stream));
        std::vector<JobSpec> specs;
        for (size_t q = c.q0; q < c.q1; q++) {
            Align* a = units[q].a;
            const size_t o = c.roff[q - q0];
            for (int e = 0; e < a->E; e++) specs.push_back(a->job(e, units[q].states, c.d_ra + o, c.d_rl + o, c.d_ri + o, ob.as<JobOut>() + specs.size()));
        }
        PS_TRY(c.b.build(rt, specs, 1, 0));
        // MapAlignments ends with updaterefs (cpp/EventUtil.cpp:51), and so does EventData::setData of a copy's AlignData (cpp/EventData.h:223)
        PS_TRY(launch_updaterefs(rt, c.b.d));
        if (tk) tk->lap("seed batch build");
        const int rc = realign(rt, c.b, n > 1 ? PLAN_OVER_GUESS * cap : 0.0);
        if (rc == PS_SPLIT) {   // wider bands than guessed: cut the chunk again with the width it asked for
            if (trace_on()) fprintf(stderr, "[ps] %s chunk of %zu cut again: %d slots per anti-diagonal, %d guessed\n", what, n, c.b.P, p_seen);
            p_seen = std::max(p_seen, c.b.P);
            limit = std::max<size_t>(1, n / 2);
            PS_HIP(hipStreamSynchronize(rt->stream));
            rt->stage.release(stage_mark);
            continue;
        }
        PS_TRY(rc);
        p_seen = std::max(p_seen, c.b.P);
        PS_TRY(collect(c));
        rt->stage.release(stage_mark);   // the stream is idle: this chunk's staging memory can be reused
        if (nchunks) ++*nchunks;
        q0 = c.q1;
    }
    return PS_OK;
}

}  // namespace ps
