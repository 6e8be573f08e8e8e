// stx_modes.cpp — the process-wide modes: which sinf / cosf the projectors follow (stx_device_math.h), the interpolation
// model of the image samples, the pyrDown order of the fp32 weight pyramids, where the exposure gain systems are solved
// (include/stitching_amd.h).  Process-wide like the libm they stand for; each is initialised from its environment variable on first use and set by its stx_set_* call afterwards.
#include <cstdlib>
#include <cstring>

#include "stx_internal.h"

namespace {

// one mode: -1 until first read, then what parse(getenv(env)) gave — unless a stx_set_* call stored a value first
struct Mode {
    const char* env;
    int (*parse)(const char* e);
    std::atomic<int> v{-1};
    int now()
    {
        int m = v.load();
        if (m >= 0) return m;
        int expected = -1;
        v.compare_exchange_strong(expected, parse(getenv(env)));
        return v.load();
    }
};

// STITCHING_AMD_TRIG = exact | glibc | glibc-nofma
int parse_trig(const char* e)
{
    if (e && !strcmp(e, "glibc")) return STX_TRIG_GLIBC;
    if (e && !strcmp(e, "glibc-nofma")) return STX_TRIG_GLIBC_NOFMA;
    if (e && *e && strcmp(e, "exact")) fprintf(stderr, "[stitching_amd] STITCHING_AMD_TRIG=%s is not one of exact, glibc, glibc-nofma: using exact\n", e);
    return STX_TRIG_EXACT;
}

// STITCHING_AMD_REMAP = q15 | float | float-fma
int parse_remap(const char* e)
{
    if (e && !strcmp(e, "float")) return STX_REMAP_FLOAT;
    if (e && !strcmp(e, "float-fma")) return STX_REMAP_FLOAT_FMA;
    if (e && *e && strcmp(e, "q15")) fprintf(stderr, "[stitching_amd] STITCHING_AMD_REMAP=%s is not one of q15, float, float-fma: using q15\n", e);
    return STX_REMAP_Q15;
}

// STITCHING_AMD_PYRDOWN ("simd-hv", "simd-v-fma:8", ...); packed as mode | lanes << 8
int parse_pyrdown(const char* e)
{
    int mode = STX_PYRDOWN_SCALAR, lanes = 4;
    if (e && *e) {
        std::string v(e);
        const size_t colon = v.find(':');
        if (colon != std::string::npos) { lanes = atoi(v.c_str() + colon + 1); v.resize(colon); }
        if (v == "simd-v") mode = STX_PYRDOWN_SIMD_V;
        else if (v == "simd-hv") mode = STX_PYRDOWN_SIMD_HV;
        else if (v == "simd-v-fma") mode = STX_PYRDOWN_SIMD_V | STX_PYRDOWN_FMA;
        else if (v == "simd-hv-fma") mode = STX_PYRDOWN_SIMD_HV | STX_PYRDOWN_FMA;
        else if (v != "scalar") fprintf(stderr, "[stitching_amd] STITCHING_AMD_PYRDOWN=%s is not scalar, simd-v, simd-hv, simd-v-fma or simd-hv-fma: using scalar\n", e);
        if (lanes != 4 && lanes != 8 && lanes != 16) { fprintf(stderr, "[stitching_amd] STITCHING_AMD_PYRDOWN lanes %d: using 4\n", lanes); lanes = 4; }
    }
    return mode | (lanes << 8);
}

// STITCHING_AMD_EXPOSURE_SOLVER = host | device
int parse_exposure_solver(const char* e)
{
    if (e && !strcmp(e, "device")) return STX_EXPOSURE_SOLVER_DEVICE;
    if (e && *e && strcmp(e, "host")) fprintf(stderr, "[stitching_amd] STITCHING_AMD_EXPOSURE_SOLVER=%s is not one of host, device: using host\n", e);
    return STX_EXPOSURE_SOLVER_HOST;
}

Mode g_exposure_solver{"STITCHING_AMD_EXPOSURE_SOLVER", parse_exposure_solver};
Mode g_trig{"STITCHING_AMD_TRIG", parse_trig}, g_remap{"STITCHING_AMD_REMAP", parse_remap}, g_pyrdown{"STITCHING_AMD_PYRDOWN", parse_pyrdown};

}  // namespace

int trig_mode_now() { return g_trig.now(); }
int remap_mode_now() { return g_remap.now(); }
int pyrdown_now() { return g_pyrdown.now(); }
int exposure_solver_now() { return g_exposure_solver.now(); }

STX_EXPORT int stx_get_trig_mode(void) { return trig_mode_now(); }

STX_EXPORT int stx_set_trig_mode(int mode)
{
    if (mode < STX_TRIG_EXACT || mode > STX_TRIG_GLIBC_NOFMA) return stx_fail(STX_ERR_INVALID, "trig mode %d", mode);
    g_trig.v.store(mode);  // (ROI cache entries carry their mode in the key)
    return STX_OK;
}

STX_EXPORT int stx_get_remap_mode(void) { return remap_mode_now(); }

STX_EXPORT int stx_set_remap_mode(int mode)
{
    if (mode < STX_REMAP_Q15 || mode > STX_REMAP_FLOAT_FMA) return stx_fail(STX_ERR_INVALID, "remap mode %d", mode);
    g_remap.v.store(mode);
    return STX_OK;
}

STX_EXPORT int stx_get_pyrdown_mode(int* out_lanes)
{
    const int m = pyrdown_now();
    if (out_lanes) *out_lanes = m >> 8;
    return m & 255;
}

STX_EXPORT int stx_set_pyrdown_mode(int mode, int lanes)
{
    const bool known = mode == STX_PYRDOWN_SCALAR || (mode & ~STX_PYRDOWN_FMA) == STX_PYRDOWN_SIMD_V || (mode & ~STX_PYRDOWN_FMA) == STX_PYRDOWN_SIMD_HV;
    if (!known || (lanes != 4 && lanes != 8 && lanes != 16)) return stx_fail(STX_ERR_INVALID, "pyrDown mode %d, lanes %d", mode, lanes);
    g_pyrdown.v.store(mode | (lanes << 8));
    return STX_OK;
}

STX_EXPORT int stx_get_exposure_solver(void) { return exposure_solver_now(); }

STX_EXPORT int stx_set_exposure_solver(int mode)
{
    if (mode != STX_EXPOSURE_SOLVER_HOST && mode != STX_EXPOSURE_SOLVER_DEVICE) return stx_fail(STX_ERR_INVALID, "exposure solver %d", mode);
    g_exposure_solver.v.store(mode);
    return STX_OK;
}
