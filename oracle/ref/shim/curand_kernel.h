// curand_kernel.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/).
//
// cuRAND is the one part of the hot path the reference does not contain (an NVIDIA library). The
// generator here is THIS PROJECT'S restatement of cuRAND's XORWOW (csrc/iq_xorwow.h), pinned only by
// rocRAND's jump tables and SURVEY.md §8c's known-answer vector; the reference build therefore proves
// nothing about the generator itself, only about how the reference consumes it.
#pragma once
#include "cuda_runtime.h"
#include "iq_xorwow.h"

struct curandStateXORWOW { iq_xorwow_state s; };
typedef curandStateXORWOW curandState;
typedef curandStateXORWOW curandState_t;

inline const uint32_t* ref_shim_xorwow_tables() {
    static const struct tables_t {
        uint32_t t[32 * IQ_XORWOW_MAT_WORDS];
        tables_t() { iq_xorwow_subseq_tables(t, 32); }
    } tables;
    return tables.t;
}

// offset is always 0 in the reference (path_tracer.cu: "no offset"); anything else is not restated
inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset,
                        curandState* state) {
    if (offset != 0) std::abort();
    iq_xorwow_init(seed, subsequence, ref_shim_xorwow_tables(), 32, &state->s);
}
inline unsigned int curand(curandState* state) { return iq_xorwow_next(&state->s); }
