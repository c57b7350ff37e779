// The knob sets of ops_api.cpp for the sanitizer harnesses that do not link it: stubs.cpp's launch_igemm asks igemm_plan under tune().  Default knobs.
#include "../../consolver_amd/csrc/ops.h"
TuneSet g_tune;
thread_local const TuneSet* t_tune = nullptr;
