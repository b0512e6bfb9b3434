// aec_tune.h -- measurement knobs.  The library as shipped reads ONE environment variable (AEC_ABI_TRACE,
// aec_abi.cpp).  Everything else -- forced kernel variants, geometry overrides, diagnostics -- exists only in a
// build with -DAEC_TUNING (make tuning: libaec_amd/lib/tuning/libaec.so.0, loaded by the tests and benches that
// compare variants via AEC_AMD_LIB); without it the functions below return their defaults.
//
// A name is read through tune() / tune_set() only while a test, bench or script names it (tests/test_tune_knobs.py);
// a value that nothing varies is a constant where it is used.  The names:
//   AEC_IDX_SMALL=0        no every-bit scheme                                  tests/cross_scheme.py
//   AEC_IDX_REGIONS=0      no region index                                      tests/cross_scheme.py
//   AEC_IDX_REGIONS_MIN    shortest stream (bits) the region index takes        tests/cross_scheme.py, tests/narrow_cases.py
//   AEC_IDX_LOCK=0         no phase-locked chains (the 64 agreeing chains)      tests/cross_scheme.py
//   AEC_IDX_LOCK_P=0       no entries by plausibility                           tests/cross_scheme.py
//   AEC_IDX_NO_SPARSE=1    no window tables                                     tests/cross_scheme.py
//   AEC_IDX_STATS=1        what each index scheme did, on stderr (synchronises) tests/prof_regions.sh
//   AEC_S2_PROF=1          phase stamps of k_spec2 / k_spec4                    tests/collect_profiles.sh
//   AEC_DW_PROF=1          phase stamps of k_decode_wave                        tests/collect_profiles.sh
//   AEC_DEC_WAVE_MAX       most RSIs the wave decoder takes                     tests/test_foreign_predictor.py
//   AEC_ENC_LOCAL          0 / 1: never / always the local encode route         tests/enc_local_cases.py
//   AEC_ENC_LOCAL_GUESS    the route's guess rule                               tests/enc_local_cases.py
//   AEC_ENC_LOCAL_SPW      its segments per wavefront                           tests/place_rounds_cases.py
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace aec {

#ifdef AEC_TUNING
inline uint32_t tune(const char *name, uint32_t dflt)
{
    const char *e = getenv(name);
    return e ? (uint32_t)atoi(e) : dflt;
}
inline bool tune_set(const char *name) { return getenv(name) != nullptr; }
#else
inline uint32_t tune(const char *, uint32_t dflt) { return dflt; }
inline bool tune_set(const char *) { return false; }
#endif

}  // namespace aec
