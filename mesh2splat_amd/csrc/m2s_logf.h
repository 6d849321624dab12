// m2s_logf.h — the C library's logf on the device (logf_glibc and its table) for every row encoder.  The restatement itself lives in
// m2s_export.hip, next to the account of how it was proven equal to glibc's logf over all positive finite floats; this header includes
// that section of the file alone, so that there is one copy of the constants.
#pragma once
#define M2S_LOGF_SECTION_ONLY
#include "m2s_export.hip"
#undef M2S_LOGF_SECTION_ONLY
