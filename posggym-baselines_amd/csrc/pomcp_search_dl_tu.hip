// The depth-specialised k_search kernels (pomcp_search.hip, template parameter
// DL) in translation units of their own, beside pomcp_search_tu.hip.
//
// build.py compiles this file once per depth limit, -DPB_SEARCH_DL=1..kRegPath,
// in parallel with the other units and with pomcp_search_tu.hip's flags (the
// iterative ILP scheduler): each object holds the DL = PB_SEARCH_DL kernels of
// both environments, the three selection rules and both workgroup sizes, and
// pb_search_kernel_dl<DL>, which pomcp_search_tu.hip's pb_search_kernel hands on
// to the launcher.  As there, the shared device code gets a namespace of its
// own per object.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>

#ifndef PB_SEARCH_DL
#error "compile with -DPB_SEARCH_DL=1..3 (build.py)"
#endif
#if PB_SEARCH_DL == 1
#define pb pb_search_dl1
#elif PB_SEARCH_DL == 2
#define pb pb_search_dl2
#elif PB_SEARCH_DL == 3
#define pb pb_search_dl3
#else
#error "PB_SEARCH_DL: 1..3 (kRegPath)"
#endif
#include "pomcp_kernels.hip"
#include "pomcp_search.hip"
