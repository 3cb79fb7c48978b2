// api_internal.hpp -- what crosses a file boundary between the translation units of the extern "C" boundary (context.hip, srs.cpp, msm_api.cpp,
// opening.cpp, vector_api.cpp, debug_api.cpp).  State stays private to the file that owns it: only types and functions are declared here.
#pragma once
#include <map>
#include <memory>

#include "common.hpp"
#include "host_ec.hpp"
#include "msm.hpp"

namespace kh {
struct LagrangeChunk { DevBuf pts; DevBuf inf; bool has_inf = false; size_t n = 0; int precomp_c = 0; };
}  // namespace kh

struct kh_srs {
    int curve = 0;
    int device = -1;          // the device its tables live on: every entry point taking this handle runs there
    size_t n = 0;
    kh::DevBuf g;                 // window tables of g_stride = n + 2 points: g[0..n), then the slots of H and U
    size_t g_stride = 0;      // (the two extra bases of the opening rounds, written by kh_ipa_begin)
    int g_precomp_c = 0;
    kh::DevBuf g_wide; int g_wide_c = 0;   // second table set with wide windows (MSM_WIDE_C) for bases of >= msm_wide_min_n() points: big single MSMs
    bool ipa_live = false;    // the U slot belongs to one opening at a time
    std::thread::id ipa_owner;   // ... begun by this thread (a second opening from ANOTHER thread waits for it: SRS::open is re-entrant on &self)
    // workspace of the opening rounds, kept across openings (hipMalloc / hipFree cost ~0.1 ms each: 1 ms per proof)
    kh::DevBuf ipa_a[2], ipa_b[2], ipa_coef[2], ipa_sc, ipa_partial, ipa_sg;
    hipEvent_t ipa_ev = nullptr;
    // the late rounds' materialised folded basis (csrc/rebase.hip): its window tables, the materialisation's workspaces, a low-priority side stream, the
    // events that order it against the rounds, a pinned "an output was the identity" word
    kh::DevBuf ipa_rb_tab, ipa_rb_B, ipa_rb_part, ipa_rb_lists, ipa_rb_scratch;
    hipStream_t ipa_rb_stream = nullptr;
    hipEvent_t ipa_rb_go = nullptr, ipa_rb_snap = nullptr, ipa_rb_done = nullptr;
    uint32_t* ipa_rb_fail = nullptr;
    uint64_t h[8];
    // fixed-base table of the blinding base: h_table[i * 255 + (j - 1)] = j * 2^(8 i) * h (XYZZ), built on first use:
    // SRS::mask_custom is one scalar multiplication by h per chunk (ipa.rs:605-622) -- 32 additions instead of 255
    // doublings + ~128 additions (a proof masks 23 commitments: 3.5 ms of host time otherwise)
    std::vector<khost::xyzz> h_table;
    std::vector<uint64_t> h_multiples;     // 2^(c w) * h for the W windows (affine, 8 words each): slots of the opening's MSMs
    std::mutex h_mu;
    // handle-level locks (callers may be on different contexts, kh_private_context_begin): the basis map, and the one opening a handle runs at a time
    std::mutex map_mu;
    std::mutex ipa_mu; std::condition_variable ipa_cv;
    std::map<unsigned, std::vector<std::unique_ptr<kh::LagrangeChunk>>> lagrange;
    ~kh_srs() {                                                     // the DevBufs free themselves
        if (ipa_ev) (void)hipEventDestroy(ipa_ev);
        if (ipa_rb_go) (void)hipEventDestroy(ipa_rb_go);
        if (ipa_rb_snap) (void)hipEventDestroy(ipa_rb_snap);
        if (ipa_rb_done) (void)hipEventDestroy(ipa_rb_done);
        if (ipa_rb_stream) { (void)hipStreamSynchronize(ipa_rb_stream); (void)hipStreamDestroy(ipa_rb_stream); }
        if (ipa_rb_fail) (void)hipHostFree(ipa_rb_fail);
    }
};
#define KH_ON_DEVICE_OF(srs) kh::DeviceScope dev_scope_((srs) ? (srs)->device : -1)

namespace kh {
// srs.cpp
int resolve_basis(kh_srs_t* srs, int basis, unsigned chunk, MsmBasis& out);
void xyzz_to_affine_batch(const khost::Crv& crv, const std::vector<khost::xyzz>& acc, uint64_t* out_xy, uint8_t* out_inf);
// context.hip: per (host thread, device)
hipStream_t thread_copy_stream();
hipEvent_t thread_upload_event();          // kh_msm_submit_host: orders the job's first kernel behind the upload on the copy stream
// msm_api.cpp
int acquire_slot(std::unique_lock<std::mutex>* lk, Context& C, bool side_first = false);
const char* slot_error(int si);
int wait_then_finish(std::unique_lock<std::mutex>& lk, Context& C, MsmSlot& S, uint64_t* out_xy, uint8_t* out_inf);
double last_wait_us();           // spin / block part of the last wait_then_finish on this thread
// vector_api.cpp
void xfer_trim(int d);
}  // namespace kh
