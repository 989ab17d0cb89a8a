// render_units.hip — the kernel units of libpsdr_hip.so: compiled once per k = 1..10 with -DPSDR_TU=k (psdr_jit_amd/build.py), each time
// instantiating list PSDR_TU<k> of render_kernels.h and nothing else.  No host code: an edit of api.hip leaves these objects alone.
#include "render_kernels.h"

#if !defined(PSDR_TU)
#error "render_units.hip is compiled with -DPSDR_TU=1..10"
#elif PSDR_TU == 1
PSDR_TU1()
#elif PSDR_TU == 2
PSDR_TU2()
#elif PSDR_TU == 3
PSDR_TU3()
#elif PSDR_TU == 4
PSDR_TU4()
#elif PSDR_TU == 5
PSDR_TU5()
#elif PSDR_TU == 6
PSDR_TU6()
#elif PSDR_TU == 7
PSDR_TU7()
#elif PSDR_TU == 8
PSDR_TU8()
#elif PSDR_TU == 9
PSDR_TU9()
#elif PSDR_TU == 10
PSDR_TU10()
#else
#error "PSDR_TU: 1..10"
#endif
