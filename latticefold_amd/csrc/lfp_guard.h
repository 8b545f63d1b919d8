// lfp_guard.h -- the exception guard of the LatticeFold+ entry points (lfp_prover.cpp, the _dev family of lfp_capi.cpp)
#pragma once
// no C++ exception crosses the C boundary: an allocation that fails inside an entry point ends it with LFPLUS_E_HIP (the code for "a resource could not be had")
#define LFP_GUARD(expr, on_throw) try { return (expr); } catch (...) { return (on_throw); }
