// ps_batch_loop.inc — the lock-step batch entry points of include/poreseq_hip.h for the CPU checkers (TEST INFRASTRUCTURE):
// a plain loop over the single-handle calls.  Included at the end of ps_oracle.cpp and ref_shim.cpp, after their
// extern "C" single-handle functions.
//
// ps_rng: both checkers draw ViterbiMutate's deviates from libc rand() (the oracle because the reference does,
// cpp/Viterbi.cpp:108).  glibc's rand() is random() on the process-wide state, so a per-region generator is a 128-byte
// TYPE_3 state switched in with setstate() around that region's call — the stream rand() would produce after srand(seed).
#include <stdlib.h>
#include <string.h>

struct ps_rng { char st[128]; };

extern "C" {

int ps_rng_create(ps_rng** out, uint32_t seed) {
    if (!out) return PS_ERR_BAD_ARG;
    ps_rng* r = new ps_rng();
    memset(r->st, 0, sizeof(r->st));
    char* prev = initstate(seed, r->st, sizeof(r->st));
    setstate(prev);
    *out = r;
    return PS_OK;
}
void ps_rng_destroy(ps_rng* r) { delete r; }

int ps_batch_score_alignments(int32_t n, ps_align* const* a, double* const* scores, double* const* likes) {
    for (int i = 0; i < n; i++) { int rc = ps_score_alignments(a[i], scores[i], likes ? likes[i] : nullptr); if (rc) return rc; }
    return PS_OK;
}
int ps_batch_find_mutations(int32_t n, ps_align* const* a, const ps_seqs* const* seeds, ps_muts** out) {
    for (int i = 0; i < n; i++) {
        const int64_t ns = ps_seqs_count(seeds[i]), nb = ps_seqs_bytes(seeds[i]);
        std::vector<int64_t> off((size_t)ns + 1);
        std::vector<char> pool((size_t)nb + 1);
        ps_seqs_export(seeds[i], off.data(), pool.data());
        int rc = ps_find_mutations(a[i], (int32_t)ns, off.data(), pool.data(), &out[i]);
        if (rc) return rc;
    }
    return PS_OK;
}
int ps_batch_score_mutations(int32_t n, ps_align* const* a, const ps_muts* const* muts, ps_muts** out) {
    for (int i = 0; i < n; i++) { int rc = ps_score_mutations(a[i], muts[i], &out[i]); if (rc) return rc; }
    return PS_OK;
}
int ps_batch_make_mutations(int32_t n, ps_align* const* a, const ps_muts* const* scored, int32_t* n_bases) {
    for (int i = 0; i < n; i++) { int rc = ps_make_mutations(a[i], scored[i], &n_bases[i]); if (rc) return rc; }
    return PS_OK;
}
int ps_batch_viterbi_mutate(int32_t n, ps_align* const* a, ps_rng* const* rng, int32_t nkeep, double skip, double stay,
                            double mmin, double mmax, ps_seqs** out) {
    for (int i = 0; i < n; i++) {
        char* prev = (rng && rng[i]) ? setstate(rng[i]->st) : nullptr;
        int rc = ps_viterbi_mutate(a[i], nkeep, skip, stay, mmin, mmax, 0, &out[i]);
        if (prev) setstate(prev);
        if (rc) {   // the batch is refused as a whole; a refusal of the single call is renamed after this one and its region
            const std::string single = "ps_viterbi_mutate: ", msg = g_err;
            if (msg.compare(0, single.size(), single) == 0) g_err = "ps_batch_viterbi_mutate: region " + std::to_string(i) + ": " + msg.substr(single.size());
            for (int k = 0; k < i; k++) { ps_seqs_destroy(out[k]); out[k] = nullptr; }
            return rc;
        }
    }
    return PS_OK;
}

}  // extern "C"
