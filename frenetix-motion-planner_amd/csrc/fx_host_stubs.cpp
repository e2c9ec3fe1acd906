// Stubs of everything fx_kernels.hip defines for the host files, made from the one list of their names (FX_LAUNCHERS, fx_launch.h),
// for programs that link the library's HOST code without its device code: the sanitizer build (make asan; tools/asan_host.sh), where
// nothing launches a kernel and a stub reports hipErrorNotSupported, and the stand-alone test programs (tests/context_owners.cpp,
// tests/batch_staging.cpp, tests/materialise_staging.cpp), which build this file with -DFX_STUB_RESULT=hipSuccess.
// The stubs are WEAK definitions: a test program overrides a launcher by defining it, and takes the stubs for all the others.
#include "fx_launch.h"

#ifndef FX_STUB_RESULT
#define FX_STUB_RESULT hipErrorNotSupported
#endif

// (the header declares the launchers with their parameters: a stub is defined under a name of its own and carries the launcher's symbol)
#define FX_STUB(name)                                                                    \
    extern "C" __attribute__((weak)) hipError_t stub_##name(...) __asm__(#name);         \
    extern "C" hipError_t stub_##name(...) { return FX_STUB_RESULT; }
FX_LAUNCHERS(FX_STUB)
