/*
 * host_query.hip -- the queries and setters that plan nothing: the ABI version, the wavelet and
 * mode tables, packed shapes, the error state's readers, the workspace's one-time initialisation
 * and the resident launch's knobs.  (The switches prune_impl reads sit beside it, host_prune.hip.)
 */
#include "wtp_host.h"

using namespace wtp;

/* PyWavelets' signal-extension modes (dwt_pruning.py:35, the `mode` argument), by WTP_MODE_* id */
static const char* const g_mode_names[] = {"periodization", "zero", "constant", "symmetric", "reflect", "periodic",
                                           "smooth", "antisymmetric", "antireflect"};
constexpr int N_MODE_NAMES = (int)(sizeof g_mode_names / sizeof g_mode_names[0]);

extern "C" {

int wtp_abi_version(void) { return WTP_ABI_VERSION; }
int wtp_wavelet_count(void) { return wavelet_count(); }
const char* wtp_wavelet_name(int wid) { return wavelet_name(wid); }
int wtp_wavelet_id(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < wavelet_count(); ++i)
        if (strcmp(name, wavelet_name(i)) == 0) return i;
    return -1;
}
int wtp_dec_len(int wid) { return wavelet_flen(wid); }
int wtp_max_level(int64_t data_len, int dec_len) { return max_level(data_len, dec_len); }

int wtp_mode_id(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < N_MODE_NAMES; ++i)
        if (strcmp(name, g_mode_names[i]) == 0) return i;
    return -1;
}
const char* wtp_mode_name(int mode_id) { return (mode_id >= 0 && mode_id < N_MODE_NAMES) ? g_mode_names[mode_id] : nullptr; }

int wtp_packed_shape(int64_t H, int64_t W, int level, int64_t* rows, int64_t* cols) {
    if (level < 0 || level > 32 || !rows || !cols) return fail(WTP_EARG, -1, "bad packed-shape request");
    wt_level_geom g;
    wt_geom(H, W, level, &g);
    *rows = g.PR;
    *cols = g.PC;
    return WTP_OK;
}
int wtp_packed_shape_mode(int64_t H, int64_t W, int wavelet_id, int level, int mode_id, int64_t* rows, int64_t* cols) {
    if (level < 0 || level > 32 || !rows || !cols || H < 1 || W < 1) return fail(WTP_EARG, -1, "bad packed-shape request");
    if (!wavelet_known(wavelet_id)) return fail(WTP_EBADWAVELET, -1, "Unknown wavelet name");
    int rc = mode_check(mode_id, 0);
    if (rc != WTP_OK) return rc;
    const int F = wavelet_flen(wavelet_id);
    if (level > 0 && !wtm_levels_ok(H, W, level, F, mode_id)) return fail(WTP_EARG, -1, "bad packed-shape request");
    wt_level_geom g;
    wtm_geom(H, W, level, F, level > 0 ? mode_id : 0, &g);
    *rows = g.PR;
    *cols = g.PC;
    return WTP_OK;
}

const char* wtp_last_error(void) { return g_err.c_str(); }
int wtp_last_error_tensor(void) { return g_err_tensor; }

int wtp_workspace_init(void* ws, size_t bytes, wtp_stream_t stream) {
    if (!ws && bytes) return fail(WTP_EARG, -1, "null workspace");
    if (bytes && hipMemsetAsync(ws, 0, bytes, (hipStream_t)stream) != hipSuccess)
        return fail(WTP_EHIP, -1, "hipMemsetAsync failed");
    return WTP_OK;
}

int wtp_resident_capacity(void) { return resident_capacity(); }
int wtp_set_interior(int mode) { return fb_set_interior(mode); }
unsigned wtp_set_resident_timeout_us(unsigned us) { return set_resident_timeout_us(us); }
int wtp_set_resident_early(int mode) {
    if (mode < 0 || mode > 2) return fail(WTP_EARG, -1, "bad resident early-store mode %d", mode);
    return set_resident_early(mode);
}
int wtp_resident_early_counts(void* ws, wtp_stream_t stream, unsigned long long* early, unsigned long long* deferred) {
    if (!ws || !early || !deferred) return fail(WTP_EARG, -1, "bad early-count request");
    SelHeader* head = reinterpret_cast<SelHeader*>(ws); /* Layout::sel = 0 */
    uint32_t c[2] = {0u, 0u};
    hipStream_t s = (hipStream_t)stream;
    if (hipMemcpyAsync(c, &head->early_ws, sizeof(c), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemsetAsync(&head->early_ws, 0, sizeof(c), s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return fail(WTP_EHIP, -1, "reading the early-store counters failed");
    *early = c[0];
    *deferred = c[1];
    return WTP_OK;
}
int wtp_set_kernel_stamps(unsigned long long* stamps_dev) {
    set_kernel_stamps(stamps_dev);
    return WTP_OK;
}

}  // extern "C"
