// libhipfeat: C ABI (include/hipfeat.h) + kernel dispatch.  gfx950 only; no torch, no Python.
#include "../../include/hipfeat.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <variant>
#include <vector>

#include "common.hpp"
#include "kernel_generic.hpp"
#include "fft512_common.hpp"
#include "kernel_fft512b.hpp"
#include "kernel_fft512c.hpp"
#include "kernel_fft1024c.hpp"
#include "kernel_fft2048c.hpp"
#include "plan_tables.hpp"
#include "kernel_resample.hpp"
#include "resample_tables.hpp"
#include "kernel_minibatch.hpp"
#include "kernel_mix.hpp"
#include "kernel_reverb.hpp"
#include "kernel_reverb_fft.hpp"
#include "kernel_collate.hpp"
#include "kernel_featmix.hpp"
#include "kernel_stats.hpp"
#include "stats_tables.hpp"
#include "kernel_level.hpp"
#include "kernel_sinc.hpp"
#include "kernel_specaug.hpp"
#include "kernel_whisper2.hpp"
#include "kernel_whisper3.hpp"
#include "layout_rounds.hpp"
#include "ticket_slots.hpp"
#include "kernel_fft256.hpp"
#include "kernel_fft256c.hpp"
#include "kernel_wave.hpp"
#include "kernel_stft.hpp"
#include "kernel_stream.hpp"
#include "kernel_grad.hpp"
#include "grad_tables.hpp"
#include "host_bulk.hpp"

using namespace hipfeat;

// --------------------------------------------------------------------------------------
// error plumbing
// --------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

// Environment switches, two classes:
//   route_env  ROUTING switches choose among kernels / launch routes that ALL meet the parity bar (HIPFEAT_FORCE_GENERIC, *_VARIANT,
//              HIPFEAT_NO_FIXED_SCHEDULE, HIPFEAT_NO_WAVE_*, HIPFEAT_NO_FLAT, HIPFEAT_NO_WIDE_STORE, HIPFEAT_RESAMPLE_GENERIC / _MFMA, HIPFEAT_MB_NO_INLINE): the GPU
//              suite uses them to compare the instances of ONE library against each other, bit for bit where the arithmetic is the same.
//   exp_env    EXPERIMENT switches skip work or retune launch shapes (HIPFEAT_MB_SKIP = deliberately wrong results, HIPFEAT_MB_SLOTS,
//              HIPFEAT_ROUNDS, HIPFEAT_ROUNDS_R3).  They exist only in builds with -DHIPFEAT_EXPERIMENTS (tools/variants.py); in the
//              product library the names are never read, so no environment can make it emit wrong results.
static inline const char* route_env(const char* name) { return getenv(name); }
#ifdef HIPFEAT_EXPERIMENTS
static inline const char* exp_env(const char* name) { return getenv(name); }
#else
static inline const char* exp_env(const char*) { return nullptr; }
#endif

static hipfeat_status fail(hipfeat_status st, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return st;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return fail(HIPFEAT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorName(e_), __FILE__, __LINE__); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// --------------------------------------------------------------------------------------
// objects
// --------------------------------------------------------------------------------------
// How every entry point gets its tables to the device ("Ticketed handles"): a pinned host buffer and a device buffer of one
// capacity, and the event that says when the launches that used them last are done.
struct StagedSlot {
  void* h = nullptr;  // pinned host
  void* d = nullptr;  // device
  size_t cap = 0;
  hipEvent_t ev = nullptr;
  bool busy = false;
  hipError_t wait() {  // for the launches that used this slot's memory last time
    if (!busy) return hipSuccess;
    const hipError_t e = hipEventSynchronize(ev);
    if (e == hipSuccess) busy = false;
    return e;
  }
  hipError_t reserve(size_t bytes) {  // the event exists and both buffers hold `bytes`; their old contents are not kept
    hipError_t e = ev ? hipSuccess : hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess || cap >= bytes) return e;
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    h = d = nullptr;
    cap = 0;
    const size_t grown = std::max<size_t>(bytes * 2, 1 << 14);
    if ((e = hipHostMalloc(&h, grown, hipHostMallocDefault)) != hipSuccess) return e;
    if ((e = hipMalloc(&d, grown)) != hipSuccess) return e;
    cap = grown;
    return hipSuccess;
  }
  hipError_t record(hipStream_t st) {  // behind the launches; memory its event cannot guard is waited for here instead
    const hipError_t e = hipEventRecord(ev, st);
    busy = (e == hipSuccess);
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    return e;
  }
  void free_all() {
    if (busy && ev) (void)hipEventSynchronize(ev);
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
    if (ev) (void)hipEventDestroy(ev);
  }
};

// the slots of an entry point without tickets, taken round-robin under its owner's mutex
template <int N>
struct SlotRing {
  StagedSlot slots[N];
  int next = 0;
  StagedSlot& take() {
    StagedSlot& s = slots[next];
    next = (next + 1) % N;
    return s;
  }
  void free_all() {
    for (auto& s : slots) s.free_all();
  }
};

// the way in: the slot's last launches are done, both buffers hold `total` bytes, `fill` has written the pinned one and its first
// `copied` bytes are on their way to the device (what lies behind them is device scratch of the launches)
template <typename Fill>
static hipError_t stage(StagedSlot& s, size_t total, size_t copied, hipStream_t st, Fill fill) {
  hipError_t e = s.wait();
  if (e == hipSuccess) e = s.reserve(total);
  if (e != hipSuccess) return e;
  fill(static_cast<unsigned char*>(s.h));
  return hipMemcpyAsync(s.d, s.h, copied, hipMemcpyHostToDevice, st);
}

// the way out, behind the issued launches (e1: hipGetLastError behind them): the slot's event guards its memory, or the stream has been
// waited for
constexpr const char* kWaitedLaunch = "the launch was enqueued and has been waited for";
constexpr const char* kWaitedLaunches = "the launches were enqueued and have been waited for";
static hipfeat_status finish_launches(StagedSlot& s, hipStream_t st, hipError_t e1, const char* kind, const char* waited) {
  const hipError_t e2 = s.record(st);
  if (e1 != hipSuccess) return fail(HIPFEAT_ERR_HIP, "%s launch failed: %s", kind, hipGetErrorName(e1));
  if (e2 != hipSuccess) return fail(HIPFEAT_ERR_HIP, "%s: hipEventRecord failed: %s (%s)", kind, hipGetErrorName(e2), waited);
  return HIPFEAT_OK;
}

// HIP device `device` exists, or the refusal is written
static hipfeat_status check_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return fail(HIPFEAT_ERR_HIP, "device %d not available (%d HIP devices visible)", device, ndev);
  return HIPFEAT_OK;
}

// The kernel family a plan runs.  hipfeat_plan_create tries the families in a fixed order; the first setup that accepts the
// configuration claims the plan, the generic kernel takes the rest.
enum class Route {
  Generic,   // generic_kernel (kernel_generic.hpp): any configuration
  Fft512b,   // fft512 "b": 16-frame tiles (fbank / mfcc / spectrogram)
  Fft256b,   // fft256 "b": 32-frame tiles
  Wave,      // wave-per-frame kernel: power-of-two fft 512 .. 2048 without a specialised kernel
  Whisper2,  // whisper: 16 x 25 mixed-radix FFT + banded mel GEMM, normalisation in a separate pass
  Fft512c,   // fft512 wave-autonomous fbank / mfcc
  Fft1024c,  // fft1024 wave-autonomous fbank
  Whisper3,  // whisper wave-autonomous with the normalisation fused
  Fft2048c,  // fft2048 wave-autonomous fbank
  Fft256c,   // fft256 wave-autonomous fbank
};

// The one argument of a plan's kernel: the Params struct of its family.  The setup that claims the plan fills every field that does not
// depend on the call, straight from the tables it built; launch() copies it and binds the buffers and the layout.
using KernelParams = std::variant<GenericParams, WaveParams, Whisper2Params, Whisper3Params, Fft512Params, Fft512cParams, Fft1024cParams, Fft2048cParams>;

struct hipfeat_plan {
  hipfeat_config cfg{};
  int device = 0;
  int feature_dim = 0;
  int npad_left = 0;
  std::string kernel_name = "generic";
  int blocks_per_cu = 0;  // hipOccupancyMaxActiveBlocksPerMultiprocessor for the selected kernel
  // the launch, recorded by the setup that claims the plan: one workgroup per layout workgroup
  Route route = Route::Generic;
  const void* fn = nullptr;       // kernel instance
  const void* fn_flat = nullptr;  // fft512c: the FLAT instance of ragged batches (nullptr: none)
  // fft512c with the 16-byte feature store: the one-dword-per-frame twins of fn / fn_flat, launched where the layout's row stride is
  // kMel4WideMaxStride or more (the wide store's 32-bit lane offset holds three rows and a column only below it); nullptr: fn / fn_flat serve all
  const void* fn_far = nullptr;
  const void* fn_flat_far = nullptr;
  int block = 0;        // threads per workgroup
  size_t lds = 0;       // dynamic LDS bytes
  KernelParams params;  // (the generic kernel's until a setup claims the plan)
  std::vector<void*> uploads;  // the device tables `params` points to, in upload order: the plan's to free
  // frames per workgroup.  Wave-autonomous kernels: fpb_unit (frames of one round of all waves) x rounds, rounds chosen per LAYOUT between 2
  // and c_rounds_max: long launches take many rounds per workgroup (the constant tables and the first, un-overlapped span are paid once per
  // workgroup: 16 instead of 8 rounds is + 4 % on the bench workload), short ones few (enough workgroups to fill the chip)
  int fpb = 8;
  int fpb_unit = 0, c_rounds_max = 0;
  // transient-layout staging ring (hipfeat_extract)
  mutable std::mutex mu;
  mutable SlotRing<4> ring;
  // host-form scratch (hipfeat_extract_host)
  mutable float* d_scratch_wave = nullptr;
  mutable size_t scratch_wave_cap = 0;
  mutable float* d_scratch_out = nullptr;
  mutable size_t scratch_out_cap = 0;
};

struct hipfeat_layout {
  int device = 0;
  int64_t batch = 0;
  int64_t total_frames = 0;
  int64_t total_blocks = 0;
  int64_t out_row_stride = 0;
  int uniform_bpc = 0;
  int fpb = 0, fpb_unit = 0;
  CutDesc* d_cuts = nullptr;
  bool owns = true;
  std::vector<int64_t> num_frames;
  std::vector<int32_t> block_cut;  // ragged batches: owner of every workgroup (uploaded behind the descriptors; uniform_bpc = -1)
  bool flat = false;               // ragged batch laid out by frame quads (fft512c FLAT instances): first_block = a cut's first quad
  int64_t total_quads = 0;
  // Whisper3: per-cut normalisation scratch behind the descriptors, kNormSlots copies handed out round-robin so that
  // launches of one layout that overlap on different streams do not share one (each copy re-arms itself at the end of its launch)
  // copy k: [total_blocks][2] float workgroup statistics, then [batch] uint32 completion counters (armed = 0)
  unsigned char* d_norm = nullptr;
  int norm_slots = 0;
  mutable std::atomic<unsigned> norm_next{0};
};
constexpr int kNormSlots = 4;
static size_t norm_slot_bytes(const hipfeat_layout* lay) { return (2 * (size_t)lay->total_blocks + (size_t)lay->batch) * 4; }

// --------------------------------------------------------------------------------------
// library / pure helpers
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_API int32_t hipfeat_abi_version(void) { return HIPFEAT_ABI_VERSION; }
extern "C" HIPFEAT_API const char* hipfeat_last_error(void) { return g_err; }

extern "C" HIPFEAT_API hipfeat_status hipfeat_device_count(int32_t* count) {
  if (!count) return fail(HIPFEAT_ERR_INVALID, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(HIPFEAT_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorName(e));
  }
  *count = n;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API int64_t hipfeat_num_frames(int64_t num_samples, int32_t frame_length, int32_t frame_shift,
                                      int32_t snip_edges) {
  if (frame_shift <= 0 || frame_length <= 0 || num_samples < 0) return 0;
  if (snip_edges) return num_samples < frame_length ? 0 : 1 + (num_samples - frame_length) / frame_shift;
  return (num_samples + frame_shift / 2) / frame_shift;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_check_length(int64_t padded_len, int32_t frame_length, int32_t frame_shift,
                                               int32_t snip_edges) {
  if (snip_edges) return HIPFEAT_OK;
  const int64_t t = hipfeat_num_frames(padded_len, frame_length, frame_shift, 0);
  if (t <= 0)
    return fail(HIPFEAT_ERR_TOO_SHORT, "waveform of %lld samples yields no frames", (long long)padded_len);
  const int64_t npad_left = (frame_length - frame_shift) / 2;
  const int64_t npad_right = (t - 1) * frame_shift + frame_length - padded_len - npad_left;
  if (npad_left > padded_len || npad_right > padded_len)
    return fail(HIPFEAT_ERR_TOO_SHORT,
                "waveform of %lld samples is shorter than the reflect padding (%lld left, %lld right)",
                (long long)padded_len, (long long)npad_left, (long long)npad_right);
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// plan
// --------------------------------------------------------------------------------------
template <typename T>
static hipfeat_status upload(T** dst, const T* src, size_t n) {
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(dst), std::max<size_t>(n, 1) * sizeof(T)));
  if (n) HIP_TRY(hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
  return HIPFEAT_OK;
}

// ... into a Params field of a handle that frees its tables as a whole: the allocation joins `owned` (a failed copy's too)
template <typename T>
static hipfeat_status upload(std::vector<void*>& owned, const T*& dst, const T* src, size_t n) {
  T* d = nullptr;
  const hipfeat_status st = upload(&d, src, n);
  if (d) owned.push_back(d);
  dst = d;
  return st;
}

static void free_uploads(std::vector<void*>& owned) {
  for (void* d : owned) (void)hipFree(d);
  owned.clear();
}

static void plan_free(hipfeat_plan* p) {
  if (!p) return;
  DeviceGuard g(p->device);
  free_uploads(p->uploads);
  (void)hipFree(p->d_scratch_wave);
  (void)hipFree(p->d_scratch_out);
  p->ring.free_all();  // (waits for the launches that used a slot)
  delete p;
}

// --------------------------------------------------------------------------------------
// specialised kernels.  Every setup_* checks that the configuration and the routing switches admit its kernel family, has the family's
// constant tables built (plan_tables.hpp: pure host code, tested on the CPU), tests the LDS budget, picks the kernel instance, fills
// a Params of the family -- each table uploaded into the field that points to it, each constant written from the tables struct -- and
// claims the plan with it.  The one place a family's kernel constants are wired is its setup: launch() adds only what a call brings.
// A setup that leaves the plan unclaimed has changed nothing the next one reads.
// --------------------------------------------------------------------------------------
template <auto* F>
static const void* entry() {
  return reinterpret_cast<const void*>(F);
}

static std::string strf(const char* fmt, ...) {
  char buf[192];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return buf;
}

// The dynamic-LDS limit of a kernel is a property of the FUNCTION, shared by every plan of the process: it is only ever
// raised (per device), so that a later plan with a smaller footprint cannot lower it under an earlier plan's launches.
#ifdef HIPFEAT_LDS_POISON
static void set_lds_poison(size_t bytes) {
  const int n = (int)(bytes / sizeof(float));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(hipfeat::g_lds_poison_floats), &n, sizeof(n));
}
#else
static inline void set_lds_poison(size_t) {}
#endif

static hipError_t ensure_dynamic_lds(const void* fn, size_t bytes) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> high;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lk(mu);
  size_t& cur = high[{fn, dev}];
  if (bytes <= cur) return hipSuccess;
  hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) cur = bytes;
  return e;
}

static hipfeat_status set_dynamic_lds(const void* fn, size_t bytes) {
  const hipError_t e = ensure_dynamic_lds(fn, bytes);
  if (e != hipSuccess) return fail(HIPFEAT_ERR_HIP, "hipFuncSetAttribute(dynamic LDS = %zu B) failed: %s", bytes, hipGetErrorName(e));
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// The frame front end -- Kaldi frames, window, pre-emphasis, DC removal, energy, radix FFT with W_fft^k twiddles -- as the plans
// (hipfeat_plan_*), the frame / STFT handles (hipfeat_stft_*) and the streams (hipfeat_stream_*) share it on the host
// --------------------------------------------------------------------------------------
// check_device, and: the kernels are gfx950 code objects and lean on gfx950's memory pipeline (hipfeat.h, HIPFEAT_WHISPER)
static hipfeat_status require_gfx950(int device) {
  if (hipfeat_status bad = check_device(device)) return bad;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(HIPFEAT_ERR_UNSUPPORTED, "device %d is not a gfx950 (MI355X-class) GPU: libhipfeat is built for that architecture alone", device);
  return HIPFEAT_OK;
}

// W_fft^k = exp(-2 pi i k / fft) for k < count, computed in double
static std::vector<float2> fft_twiddles(int fft, int count) {
  std::vector<float2> tw((size_t)count);
  for (int k = 0; k < count; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)fft;
    tw[k] = make_float2((float)std::cos(a), (float)std::sin(a));
  }
  return tw;
}

static bool radix_fft_size(int fft) { return fft == 256 || fft == 512 || fft == 1024 || fft == 2048; }

// n1 (64 n1 complex points per frame) -> f(std::integral_constant<int, n1>): the instance of a kernel template for 2, 4, 8 or 16
template <typename F>
static const void* for_n1(int n1, F f) {
  switch (n1) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}

static int energy_flags(bool remove_dc, bool use_energy, bool raw_energy) {
  return (remove_dc ? F_REMOVE_DC : 0) | (use_energy ? F_USE_ENERGY : 0) | (raw_energy ? F_RAW_ENERGY : 0);
}
static int energy_flags(const hipfeat_stft_config& c) { return energy_flags(c.remove_dc_offset, c.want_energy, c.raw_energy); }
static int energy_flags(const hipfeat_config& c) {  // ... and what the feature epilogues read
  return energy_flags(c.remove_dc_offset, c.use_energy, c.raw_energy) | (c.use_fft_mag ? F_FFT_MAG : 0) | (c.apply_lifter ? F_LIFTER : 0);
}
static float log_energy_floor(float energy_floor) { return energy_floor > 0.0f ? logf(energy_floor) : -INFINITY; }

// The rules of hipfeat_config that hipfeat_plan_create and hipfeat_stream_create_features both apply, in the plan's order; what only one
// of them refuses (whisper / librosa constraints, the streaming kernel's kinds and sizes) stays in that entry point
constexpr const char* kNeedMel = "fbank/mfcc need num_filters>0 and a mel matrix";
static hipfeat_status check_feature_config(const hipfeat_config* cfg, const float* h_window, const float* h_mel, const float* h_dct, const float* h_lifter) {
  if (cfg->struct_size != (int32_t)sizeof(hipfeat_config))
    return fail(HIPFEAT_ERR_INVALID, "hipfeat_config.struct_size %d != %zu (ABI mismatch)", cfg->struct_size, sizeof(hipfeat_config));
  const int N = cfg->frame_length, shift = cfg->frame_shift, fft = cfg->fft_length;
  if (cfg->kind < 0 || cfg->kind > 5) return fail(HIPFEAT_ERR_INVALID, "unknown kind %d", cfg->kind);
  if (N <= 0 || shift <= 0 || fft < N)
    return fail(HIPFEAT_ERR_INVALID, "need frame_length>0, frame_shift>0, fft_length>=frame_length (got %d, %d, %d)", N, shift, fft);
  if (shift > N) return fail(HIPFEAT_ERR_UNSUPPORTED, "frame_shift (%d) > frame_length (%d) is not supported", shift, N);
  if (!h_window) return fail(HIPFEAT_ERR_INVALID, "window is NULL");
  if (cfg->dither != 0.0f)
    return fail(HIPFEAT_ERR_UNSUPPORTED, "dither != 0 is not supported by the library (ABI v%d): the host adds it to the samples", HIPFEAT_ABI_VERSION);
  if ((cfg->kind == HIPFEAT_FBANK || cfg->kind == HIPFEAT_MFCC) && (cfg->num_filters <= 0 || !h_mel)) return fail(HIPFEAT_ERR_INVALID, kNeedMel);
  if (cfg->kind == HIPFEAT_MFCC) {
    if (cfg->num_ceps <= 0 || !h_dct) return fail(HIPFEAT_ERR_INVALID, "mfcc needs num_ceps>0 and a dct matrix");
    if (cfg->apply_lifter && !h_lifter) return fail(HIPFEAT_ERR_INVALID, "apply_lifter set but lifter is NULL");
  }
  return HIPFEAT_OK;
}

// columns of a feature row
static int feature_dim(const hipfeat_config& c) {
  if (c.kind == HIPFEAT_FBANK) return c.num_filters + (c.use_energy ? 1 : 0);
  if (c.kind == HIPFEAT_MFCC) return c.num_ceps;
  return (c.kind == HIPFEAT_WHISPER || c.kind == HIPFEAT_LIBROSA_FBANK) ? c.num_filters : c.fft_length / 2 + 1;
}

// The WaveParams fields (kernel_wave.hpp) that come from the config and the tables' sizes; the creator uploads the tables into the
// pointer fields and sets frames per wave and npad_left, the call brings its buffers and batch
static void fill_wave_front(WaveParams& wp, const hipfeat_config& c, const WaveTables& t) {
  const bool librosa = c.kind == HIPFEAT_LIBROSA_FBANK;
  wp.mel_blob_floats = (int)t.blob.size();
  wp.dct_in_lds = t.dct_in_lds ? 1 : 0;
  wp.N = c.frame_length;
  wp.shift = c.frame_shift;
  wp.H = c.fft_length / 2;
  wp.K = c.fft_length / 2 + 1;
  wp.M = c.kind >= HIPFEAT_FBANK ? c.num_filters : 0;
  wp.C = c.kind == HIPFEAT_MFCC ? c.num_ceps : 0;
  wp.kind = librosa ? (int)HIPFEAT_FBANK : c.kind;
  wp.flags = energy_flags(c) | (librosa ? (F_CENTER | F_LOG10) : 0);
  wp.preemph = c.preemph_coeff;
  wp.log_energy_floor = log_energy_floor(c.energy_floor);
  wp.mel_floor = c.mel_floor;
  wp.log_offset = c.log_offset;
}

// One check of hipfeat_stft_config for hipfeat_stft_create and hipfeat_stream_create_stft, which also yields n1: the spectrum's fft / 128,
// for frames the smallest of 2, 4, 8, 16 that holds the frame.  A stream (`streaming`) refuses a shift longer than the frame as well.
static hipfeat_status check_stft_config(const hipfeat_stft_config* cfg, const float* h_window, bool streaming, int* n1) {
  if (!cfg || !h_window) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (cfg->struct_size != (int32_t)sizeof(hipfeat_stft_config))
    return fail(HIPFEAT_ERR_INVALID, "hipfeat_stft_config.struct_size = %d, expected %d", (int)cfg->struct_size, (int)sizeof(hipfeat_stft_config));
  if (cfg->output != HIPFEAT_STFT_FRAMES && cfg->output != HIPFEAT_STFT_SPECTRUM) return fail(HIPFEAT_ERR_INVALID, "unknown output %d", (int)cfg->output);
  if (cfg->frame_length <= 0 || cfg->frame_shift <= 0)
    return fail(HIPFEAT_ERR_INVALID, "frame_length = %d, frame_shift = %d: both must be positive", (int)cfg->frame_length, (int)cfg->frame_shift);
  if (cfg->pad_length < cfg->frame_length)
    return fail(HIPFEAT_ERR_INVALID, "pad_length (or fft_length) = %d cannot be smaller than N = %d", (int)cfg->pad_length, (int)cfg->frame_length);
  if (streaming && cfg->frame_shift > cfg->frame_length)
    return fail(HIPFEAT_ERR_UNSUPPORTED, "frame_shift (%d) > frame_length (%d) is not supported", (int)cfg->frame_shift, (int)cfg->frame_length);
  if (cfg->output == HIPFEAT_STFT_SPECTRUM) {
    if (!radix_fft_size(cfg->pad_length))
      return fail(HIPFEAT_ERR_UNSUPPORTED, "fft_length = %d: the device front end has the sizes 256, 512, 1024 and 2048 (round_to_power_of_two=True, 8 to 48 kHz at 25 ms)",
                  (int)cfg->pad_length);
    *n1 = cfg->pad_length / 128;
  } else {
    if (cfg->frame_length > 2048) return fail(HIPFEAT_ERR_UNSUPPORTED, "frame_length = %d: the device front end holds frames of at most 2048 samples", (int)cfg->frame_length);
    for (*n1 = 2; 128 * *n1 < cfg->frame_length;) *n1 *= 2;
  }
  return HIPFEAT_OK;
}

// The front end of the STFT pair (kernel_stft.hpp on a row, kernel_stream.hpp on [context | chunk]): the config and what create made of it
struct StftFront {
  hipfeat_stft_config cfg{};
  int n1 = 0;
  size_t lds = 0;
  float* d_window = nullptr;
  float2* d_tw = nullptr;  // spectrum: W_fft^k, k < fft / 2
  bool spectrum() const { return cfg.output == HIPFEAT_STFT_SPECTRUM; }
  int width() const { return cfg.pad_length + (spectrum() ? 2 : 0); }  // floats per output row
};

static void stft_front_free(StftFront& f) {
  (void)hipFree(f.d_window);
  (void)hipFree(f.d_tw);
}

// a checked config on the current device, for the kernel instance `fn`; after a failure the caller frees
static hipfeat_status stft_front_create(StftFront& f, const hipfeat_stft_config& cfg, int n1, const float* h_window, const void* fn) {
  f.cfg = cfg;
  f.n1 = n1;
  f.lds = stft_lds_bytes(n1, cfg.output, cfg.frame_length);
  hipfeat_status st = upload(&f.d_window, h_window, (size_t)cfg.frame_length);
  if (st == HIPFEAT_OK && f.spectrum()) {
    const std::vector<float2> tw = fft_twiddles(cfg.pad_length, cfg.pad_length / 2);
    st = upload(&f.d_tw, tw.data(), tw.size());
  }
  return st == HIPFEAT_OK ? set_dynamic_lds(fn, f.lds) : st;
}

// the StftParams fields that do not depend on the call (its buffers, strides, counts and npad_left do)
constexpr int kStftFramesPerWave = 8;  // 4 waves x 8 frames per workgroup, as the wave kernel
static void fill_stft_front(StftParams& p, const StftFront& f) {
  p.window = f.d_window;
  p.tw = f.d_tw;
  p.N = f.cfg.frame_length;
  p.shift = f.cfg.frame_shift;
  p.pad = f.cfg.pad_length;
  p.frames_per_wave = kStftFramesPerWave;
  p.flags = energy_flags(f.cfg);
  p.preemph = f.cfg.preemph_coeff;
  p.log_energy_floor = log_energy_floor(f.cfg.energy_floor);
}

// The setup that accepts a configuration claims the plan with the instance it runs: the instance's dynamic-LDS limit is raised, its
// occupancy read (blocks_per_cu, part of the kernel name) and the launch recorded for launch(), `params` as the kernel's argument.
static hipfeat_status claim(hipfeat_plan* p, Route route, const void* fn, int block, size_t lds, const KernelParams& params) {
  if (hipfeat_status bad = set_dynamic_lds(fn, lds)) return bad;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, block, lds) == hipSuccess) p->blocks_per_cu = nb;
  p->route = route;
  p->fn = fn;
  p->block = block;
  p->lds = lds;
  p->params = params;
  return HIPFEAT_OK;
}

// What the Params of the wave-autonomous families (fft512c / fft256c, fft1024c, fft2048c, whisper3) share: one LDS constants image,
// uploaded here, the offsets of its tables, the filter count and floor.  The batch and the rounds of frames come with the launch.
template <typename P>
static hipfeat_status fill_wave_autonomous(P& q, hipfeat_plan* p, const WaveAutoTables& t) {
  if (hipfeat_status bad = upload(p->uploads, q.shared_consts, t.image.data(), t.image.size())) return bad;
  q.shared_floats = t.shared_floats;
  q.wtab_off = t.wtab_off;
  q.ltab_off = t.ltab_off;
  q.M = p->cfg.num_filters;
  q.mel_floor = p->cfg.mel_floor;
  return HIPFEAT_OK;
}

// Frame geometry of the wave-autonomous FFT kernels (fft512c / fft256c plans have neither magnitudes nor centred framing: their
// flags come down to F_REMOVE_DC).
template <typename P>
static void fill_frames(P& q, const hipfeat_plan* p, const WaveAutoTables& t) {
  const hipfeat_config& c = p->cfg;
  q.N = c.frame_length;
  q.shift = c.frame_shift;
  q.npad_left = p->npad_left;
  q.flags = (c.remove_dc_offset ? F_REMOVE_DC : 0) | (c.use_fft_mag ? F_FFT_MAG : 0) | (c.kind == HIPFEAT_LIBROSA_FBANK ? (F_CENTER | F_LOG10) : 0);
  q.preemph = c.preemph_coeff;
  q.xs_floats = t.xs_floats;
}

// fft1024c / fft2048c: the accumulator sets the kernel walks, every entry of the tables' arrays
template <typename P>
static void fill_sets(P& q, const WaveAutoTables& t) {
  static_assert(sizeof(q.steps) == sizeof(t.w_steps) && sizeof(q.step0) == sizeof(t.w_step0), "the kernel's set arrays and the tables' differ in length");
  q.nsets = t.w_nsets;
  std::copy(std::begin(t.w_steps), std::end(t.w_steps), q.steps);
  std::copy(std::begin(t.w_step0), std::end(t.w_step0), q.step0);
}
static_assert(kWMaxSets == kXMaxSets, "fft1024c and fft2048c take their sets from one WaveAutoTables");

// Wave-autonomous families: claims the plan for `fn` with the filled `params` and names it `head` + the common trailer.  A wave takes
// `frames` frames per round; a workgroup runs 2 .. rounds_max rounds, chosen per layout (build_descs).
static hipfeat_status claim_wave_auto(hipfeat_plan* p, Route route, const void* fn, const WaveAutoTables& t, const KernelParams& params, int frames, int rounds,
                                      int rounds_max, const std::string& head) {
  p->fpb_unit = t.waves * frames;
  p->fpb = p->fpb_unit * rounds;
  p->c_rounds_max = rounds_max;
  if (hipfeat_status bad = claim(p, route, fn, 64 * t.waves, t.lds, params)) return bad;
  p->kernel_name = head + strf(" lds=%zuB blocks/CU=%d mel4=%dx%d", t.lds, p->blocks_per_cu, t.sch_nsets, t.sch_steps);
  return HIPFEAT_OK;
}

// fft512 "b" / fft256 "b": fills the Fft512Params, uploading the tables, and claims the plan for `fn`
static hipfeat_status claim_tile(hipfeat_plan* p, Route route, const void* fn, const TileTables& t, int tile_frames, const char* kernel) {
  const hipfeat_config& c = p->cfg;
  const bool mfcc = c.kind == HIPFEAT_MFCC, spec = c.kind == HIPFEAT_SPECTROGRAM || c.kind == HIPFEAT_LOG_SPECTROGRAM;
  Fft512Params q{};
  const float* mel_a_plain = nullptr;  // fft512 "b": the operands before the reorder to mel_a (uploaded, read by no kernel)
  hipfeat_status st;
  if ((st = upload(p->uploads, q.lds_consts, t.consts.data(), t.consts.size())) != HIPFEAT_OK) return st;
  if (route == Route::Fft512b && (st = upload(p->uploads, mel_a_plain, t.mel_a.data(), t.mel_a.size())) != HIPFEAT_OK) return st;
  if ((st = upload(p->uploads, q.work, t.work, 4)) != HIPFEAT_OK) return st;
  if ((st = upload(p->uploads, q.mel_a, t.mel_a4.data(), t.mel_a4.size())) != HIPFEAT_OK) return st;
  if (mfcc && (st = upload(p->uploads, q.dct_consts, t.dct.data(), t.dct.size())) != HIPFEAT_OK) return st;
  // 16 tiles per workgroup: the constant-table load and the first, un-overlapped span fetch are paid once per workgroup (measured on
  // MI355X, cuts/s: fft512 4 -> 1.98 M, 8 -> 2.11 M, 16 -> 2.16 M; fft256 at 8 kHz fbank-80 8 -> 3.84 M, 16 -> 3.99 M, 32 -> 3.93 M)
  q.tiles_per_block = 16;
  p->fpb = tile_frames * q.tiles_per_block;
  q.N = c.frame_length;
  q.shift = c.frame_shift;
  q.npad_left = p->npad_left;
  q.M = c.num_filters;
  q.flags = (c.remove_dc_offset ? F_REMOVE_DC : 0) | (c.use_fft_mag ? F_FFT_MAG : 0) | (c.kind == HIPFEAT_LOG_SPECTROGRAM ? F_LOG_SPEC : 0);
  q.log_offset = c.log_offset;
  q.preemph = c.preemph_coeff;
  q.mel_floor = c.mel_floor;
  q.xs_floats = t.xs_floats;
  q.const_floats = (int)t.consts.size();
  q.C = c.num_ceps;
  q.lm_stride = t.lm_stride;
  q.dct_groups = t.dct_groups;
  q.dct_floats = (int)t.dct.size();
  if ((st = claim(p, route, fn, 256, t.lds, q)) != HIPFEAT_OK) return st;
  // same spelling as the device symbol rocprofv3 reports (modulo the space after the comma)
  p->kernel_name = strf("%s<%d,%d> %s lds=%zuB blocks/CU=%d", kernel, t.nrows, mfcc ? 1 : (spec ? 2 : 0), mfcc ? "mfcc" : (spec ? "spectrogram" : "fbank"), t.lds,
                        p->blocks_per_cu);
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// fft512: the wave-autonomous fbank / mfcc kernel (kernel_fft512c.hpp), else the 16-frame-tile kernel "b" (kernel_fft512b.hpp)
// --------------------------------------------------------------------------------------
// the (rows, frame length) that have a FLAT instance (ragged batches by frame quads, kernel_fft512c.hpp): the 25 ms @ 16 kHz default
static bool fft512c_has_flat(int nrows, int N) { return nrows == 13 && N >= 384; }

// (rows, frame length, mode) -> kernel instance
template <int MODE, bool WIDE = false, int T0 = kCMaxSteps, int T1 = kCMaxSteps>
static const void* fft512c_pick(int nrows, int N, bool flat) {
  if (flat && fft512c_has_flat(nrows, N)) return entry<fft512c_kernel<13, 12, MODE, true, WIDE, T0, T1>>();
  if (nrows == 10) return entry<fft512c_kernel<10, 0, MODE, false, WIDE, T0, T1>>();
  // 25 ms at 16 kHz (N = 400: 12 full rows of 32 samples + a partial one) gets the instance without length masks on the full rows
  if (nrows == 13 && N >= 384) return entry<fft512c_kernel<13, 12, MODE, false, WIDE, T0, T1>>();
  if (nrows == 13) return entry<fft512c_kernel<13, 0, MODE, false, WIDE, T0, T1>>();
  return entry<fft512c_kernel<16, 0, MODE, false, WIDE, T0, T1>>();
}
// wide: the transposed accumulators with one 16-byte store per lane and set (log-mel modes only); mode 0: with the steps `ts` of the
// two accumulator sets compiled in (fft512c_geom.hpp::fft512c_mel_steps)
static const void* fft512c_dispatch(int mode, int nrows, int N, bool flat, bool wide, Fft512cMelSteps ts) {
  if (wide && mode == 0 && ts.t0 == 16 && ts.t1 == 12) return fft512c_pick<0, true, 16, 12>(nrows, N, flat);
  if (wide && mode == 0 && ts.t0 == 16 && ts.t1 == 8) return fft512c_pick<0, true, 16, 8>(nrows, N, flat);
  if (wide && mode <= 1) return mode == 0 ? fft512c_pick<0, true>(nrows, N, flat) : fft512c_pick<1, true>(nrows, N, flat);
  return mode == 0 ? fft512c_pick<0>(nrows, N, flat)
                   : (mode == 1 ? fft512c_pick<1>(nrows, N, flat) : (mode == 2 ? fft512c_pick<2>(nrows, N, flat) : fft512c_pick<3>(nrows, N, flat)));
}

// Claims the plan (Route::Fft512c) when the configuration takes the wave-autonomous kernel, leaves it unclaimed when it does
// not (the caller then sets up kernel "b").
static hipfeat_status setup_fft512c(hipfeat_plan* p, const PlanInputs& in, int nrows) {
  const bool mfcc = p->cfg.kind == HIPFEAT_MFCC;
  if (mfcc && (in.M > 4 * kCDctChunks || in.C > 64 || !in.dct)) return HIPFEAT_OK;
  const WaveAutoTables t = build_fft512c_tables(in, nrows, {kCPRowStride, kCMaxSets, kCMaxSteps, kCWaves, kCRegion}, kCDctChunks, kCDctChunksSmall);
  // two workgroups of 8 waves per CU or nothing; the span request covers kCSpanPieces KiB (the LDS budget leaves a wave's span less)
  if (!t.fits || t.lds > 80 * 1024 || t.xs_floats > 256 * kCSpanPieces) return HIPFEAT_OK;
  // A filter count that is a multiple of 4 fills the four columns of a schedule slot or none of them (mel4_schedule.hpp): the log-mel
  // instances with transposed accumulators then store a lane's four columns with one 16-byte store.  HIPFEAT_NO_WIDE_STORE (routing switch)
  // keeps the one-dword-per-frame epilogue, which the other filter counts and the MFCC modes always have: same bits either way.
  const bool wide = !mfcc && t.mode <= 1 && in.M % 4 == 0 && !route_env("HIPFEAT_NO_WIDE_STORE");
  // The wide two-set instances run the schedule's own steps per set where an instance has them compiled in; the table keeps the padded
  // layout.  HIPFEAT_NO_FIXED_SCHEDULE (routing switch) keeps the instance that walks the padding too: same bits either way.
  const Fft512cMelSteps padded = {kCMaxSteps, kCMaxSteps};
  const Fft512cMelSteps ts = (wide && t.mode == 0 && !route_env("HIPFEAT_NO_FIXED_SCHEDULE")) ? fft512c_mel_steps(t.sch_nsets, t.sch_set_steps) : padded;
  // the exchange rows are read 16 bytes at a time: every wave's region starts on a 16-byte boundary
  if (t.shared_floats % 4 != 0 || t.xs_floats % 4 != 0) return fail(HIPFEAT_ERR_INVALID, "fft512c: a wave's LDS region is not 16-byte aligned");
  Fft512cParams q{};
  hipfeat_status st = fill_wave_autonomous(q, p, t);
  if (st == HIPFEAT_OK && !t.dct.empty()) st = upload(p->uploads, q.dct_tab, t.dct.data(), t.dct.size());
  if (st != HIPFEAT_OK) return st;
  fill_frames(q, p, t);
  q.C = p->cfg.num_ceps;
  // 8 waves x 8 rounds x 4 frames = 256 frames per workgroup
  st = claim_wave_auto(p, Route::Fft512c, fft512c_dispatch(t.mode, nrows, in.N, false, wide, ts), t, q, 4, 8, 16,
                       strf("fft512c_kernel<%d> %s", nrows, mfcc ? "mfcc" : "fbank"));
  if (st == HIPFEAT_OK && wide) p->kernel_name += " store=16B";
  const void** more[3] = {&p->fn_flat, &p->fn_far, &p->fn_flat_far};  // the same launch shape, chosen per layout (build_descs) / per launch
  for (int i = 0; st == HIPFEAT_OK && i < 3; ++i) {
    const bool flat = i != 1, far = i != 0;
    if ((flat && !fft512c_has_flat(nrows, in.N)) || (far && !wide)) continue;
    *more[i] = fft512c_dispatch(t.mode, nrows, in.N, flat, wide && !far, far ? padded : ts);
    st = set_dynamic_lds(*more[i], t.lds);
  }
  return st;
}

static hipfeat_status setup_fft512(hipfeat_plan* p, const PlanInputs& in) {
  const hipfeat_config& c = p->cfg;
  const char* force = route_env("HIPFEAT_FORCE_GENERIC");
  if (force && force[0] == '1') return HIPFEAT_OK;
  const bool mfcc = c.kind == HIPFEAT_MFCC;
  const bool spec = c.kind == HIPFEAT_SPECTROGRAM || c.kind == HIPFEAT_LOG_SPECTROGRAM;
  if (c.kind > HIPFEAT_MFCC || c.fft_length != 512 || (in.shift & 1) || in.N < 32 || c.use_energy || (!spec && c.use_fft_mag))
    return HIPFEAT_OK;
  if (mfcc && (in.M > 8 * kMaxDctGroups || in.C > 64)) return HIPFEAT_OK;
  const int need = (in.N + 31) / 32;
  const int nrows = need <= 10 ? 10 : (need <= 13 ? 13 : 16);
  if ((in.M + 15) / 16 > 8) return HIPFEAT_OK;  // at most 8 mel tiles of 16 filters

  if (!spec) {  // log-mel filterbank / MFCC: the wave-autonomous kernel, unless the schedule or the LDS budget says no
    const char* var = route_env("HIPFEAT_FFT512_VARIANT");
    if (!(var && var[0] == 'b')) {  // HIPFEAT_FFT512_VARIANT=b: the 16-frame-tile kernel for these too (tests compare the two)
      hipfeat_status stc = setup_fft512c(p, in, nrows);
      if (stc != HIPFEAT_OK || p->route == Route::Fft512c) return stc;
    }
  }
  const TileTables t = build_tile_tables(in, nrows, {16, kPRowStride, kMaxGroups0, kMaxGroups1, kTileFrames, kBWaveRegion, false});
  if (!t.fits || t.lds > 160 * 1024) return HIPFEAT_OK;  // -> generic kernel
  const void* fn;
  if (mfcc)
    fn = nrows == 10 ? entry<fft512b_kernel<10, 1>>() : (nrows == 13 ? entry<fft512b_kernel<13, 1>>() : entry<fft512b_kernel<16, 1>>());
  else if (spec)
    fn = nrows == 10 ? entry<fft512b_kernel<10, 2>>() : (nrows == 13 ? entry<fft512b_kernel<13, 2>>() : entry<fft512b_kernel<16, 2>>());
  else
    fn = nrows == 10 ? entry<fft512b_kernel<10, 0>>() : (nrows == 13 ? entry<fft512b_kernel<13, 0>>() : entry<fft512b_kernel<16, 0>>());
  return claim_tile(p, Route::Fft512b, fn, t, kTileFrames, "fft512b_kernel");
}

// --------------------------------------------------------------------------------------
// fft1024 wave-autonomous fbank kernel (kernel_fft1024c.hpp): 22.05 / 24 / 32 kHz Kaldi log-mel
// --------------------------------------------------------------------------------------
static hipfeat_status setup_fft1024c(hipfeat_plan* p, const PlanInputs& in) {
  const hipfeat_config& c = p->cfg;
  const int N = in.N, shift = in.shift;
  const bool librosa = c.kind == HIPFEAT_LIBROSA_FBANK;  // centred frames, |X| or |X|^2, log10 (librosa_fbank.py:66-137)
  if ((c.kind != HIPFEAT_FBANK && !librosa) || c.fft_length != 1024 || (shift & 1) || N < 32 * 17 || c.use_energy ||
      (c.use_fft_mag && !librosa) || route_env("HIPFEAT_FORCE_GENERIC") || route_env("HIPFEAT_NO_WAVE_AUTONOMOUS"))
    return HIPFEAT_OK;
  const int need = (N + 31) / 32;
  const int nrows = need <= 20 ? 20 : (need <= 26 ? 26 : 32);
  // The instance that has this configuration's mel schedule and frame geometry as compile-time constants (kernel_fft1024c.hpp), if the
  // schedule turns out to be that one: 1 = <20, 24,16,8> (24 kHz), 2 = <26, 24,16,8> (32 kHz), 3 = <20, 24,24,8> (22.05 kHz): the Kaldi default
  // with 80 filters (|X|^2, ln and Kaldi's edges compiled in); 4 = <32, 16,16,8, PLAIN> (the librosa default: n_fft 1024 @ 22.05 kHz, 80
  // slaney filters, no DC removal, no pre-emphasis); 0 = none
  static const int kFixedSteps[5][3] = {{0, 0, 0}, {24, 16, 8}, {24, 16, 8}, {24, 24, 8}, {16, 16, 8}};
  int want = 0;
  if (route_env("HIPFEAT_NO_FIXED_SCHEDULE")) want = 0;  // (routing switch: the generic instances)
  else if (nrows == 32) want = !c.remove_dc_offset && c.preemph_coeff == 0.0f ? 4 : 0;
  else if (!librosa && !c.use_fft_mag && in.M == 80 && !c.snip_edges)
    want = N == 600 && shift == 240 ? 1 : (N == 800 && shift == 320 ? 2 : (N == 551 && shift == 220 ? 3 : 0));
  // fixed-schedule instances: 12 waves per workgroup, the span buffer aliases the exchange / power region
  const WaveAutoTables t = build_fft1024c_tables(in, nrows, {kWPRowStride, kWMaxSets, kWMaxSteps, kWWaves, kWRegion}, kWSplitSteps, kWWavesFixed, want ? kFixedSteps[want] : nullptr);
  if (!t.fits || t.lds > 160 * 1024 || (t.xs_floats >> 8) > 10) return HIPFEAT_OK;
  const int fixed = t.fixed ? want : 0;
  const void* fn = fixed == 1 ? entry<fft1024c_kernel<20, 24, 16, 8>>()
                   : fixed == 2 ? entry<fft1024c_kernel<26, 24, 16, 8>>()
                   : fixed == 3 ? entry<fft1024c_kernel<20, 24, 24, 8>>()
                   : fixed == 4 ? entry<fft1024c_kernel<32, 16, 16, 8, true>>()
                   : nrows == 20 ? entry<fft1024c_kernel<20>>() : (nrows == 26 ? entry<fft1024c_kernel<26>>() : entry<fft1024c_kernel<32>>());
  Fft1024cParams q{};
  if (hipfeat_status bad = fill_wave_autonomous(q, p, t)) return bad;
  fill_frames(q, p, t);
  fill_sets(q, t);
  return claim_wave_auto(p, Route::Fft1024c, fn, t, q, 4, 8, 32, strf("fft1024c_kernel<%d> fbank%s waves=%d", nrows, fixed ? " fixed-schedule" : "", t.waves));
}

// --------------------------------------------------------------------------------------
// fft256 (8 kHz 25/10 ms frames, or <= 16 ms frames at 16 kHz): the wave-autonomous log-mel kernel (kernel_fft256c.hpp), else the
// 32-frame-tile kernel "b" (kernel_fft256.hpp)
// --------------------------------------------------------------------------------------
static hipfeat_status setup_fft256c(hipfeat_plan* p, const PlanInputs& in, int nrows) {
  const WaveAutoTables t = build_fft256c_tables(in, nrows, {kDPRowStride, kDSets, kDSteps, kDWaves, kDRegion});
  if (!t.fits || t.lds > 80 * 1024 || (t.xs_floats >> 8) > 6) return HIPFEAT_OK;  // two workgroups of 8 waves per CU or nothing
  // 25 ms at 8 kHz (N = 200: 12 full rows of 16 samples + a partial one) gets the instance without length masks on the full rows
  const void* fn = nrows == 13 ? (in.N >= 192 ? entry<fft256c_kernel<13, 12>>() : entry<fft256c_kernel<13, 0>>()) : entry<fft256c_kernel<16, 0>>();
  Fft512cParams q{};  // (without the MFCC and FLAT fields)
  if (hipfeat_status bad = fill_wave_autonomous(q, p, t)) return bad;
  fill_frames(q, p, t);
  // 8 waves x 4 rounds x 8 frames = 256 frames per workgroup
  return claim_wave_auto(p, Route::Fft256c, fn, t, q, 8, 4, 16, strf("fft256c_kernel<%d> fbank", nrows));
}

static hipfeat_status setup_fft256(hipfeat_plan* p, const PlanInputs& in) {
  const hipfeat_config& c = p->cfg;
  const bool mfcc = c.kind == HIPFEAT_MFCC;
  const bool spec = c.kind == HIPFEAT_SPECTROGRAM || c.kind == HIPFEAT_LOG_SPECTROGRAM;
  if (c.kind > HIPFEAT_MFCC || c.fft_length != 256 || (in.shift & 1) || in.N < 16 || c.use_energy || (!spec && c.use_fft_mag) ||
      route_env("HIPFEAT_FORCE_GENERIC"))
    return HIPFEAT_OK;
  if (mfcc && (in.M > 8 * kMaxDctGroups || in.C > 64)) return HIPFEAT_OK;
  const int nrows = (in.N + 15) / 16 <= 13 ? 13 : 16;
  if ((in.M + 15) / 16 > 8) return HIPFEAT_OK;  // at most 8 mel tiles of 16 filters
  if (!mfcc && !spec) {  // log-mel filterbank: the wave-autonomous kernel, unless the schedule or the LDS budget says no
    const char* var = route_env("HIPFEAT_FFT256_VARIANT");
    if (!(var && var[0] == 'b') && !route_env("HIPFEAT_NO_WAVE_AUTONOMOUS")) {  // HIPFEAT_FFT256_VARIANT=b: the 32-frame-tile kernel (tests compare the two)
      hipfeat_status stc = setup_fft256c(p, in, nrows);
      if (stc != HIPFEAT_OK || p->route == Route::Fft256c) return stc;
    }
  }
  const TileTables t = build_tile_tables(in, nrows, {8, k256PRowStride, kMaxGroups0, kMaxGroups1, k256TileFrames, k256WaveRegion, true});
  if (!t.fits || t.lds > 64 * 1024) return HIPFEAT_OK;  // keep at least two workgroups per CU; otherwise the generic kernel
  const void* fn;
  if (mfcc) fn = nrows == 13 ? entry<fft256_kernel<13, 1>>() : entry<fft256_kernel<16, 1>>();
  else if (spec) fn = nrows == 13 ? entry<fft256_kernel<13, 2>>() : entry<fft256_kernel<16, 2>>();
  else fn = nrows == 13 ? entry<fft256_kernel<13, 0>>() : entry<fft256_kernel<16, 0>>();
  return claim_tile(p, Route::Fft256b, fn, t, k256TileFrames, "fft256_kernel");
}

// --------------------------------------------------------------------------------------
// wave-per-frame kernel (kernel_wave.hpp): power-of-two fft 512 .. 2048 without a specialised kernel
// --------------------------------------------------------------------------------------
static hipfeat_status setup_wave(hipfeat_plan* p, const PlanInputs& in) {
  const hipfeat_config& c = p->cfg;
  const bool librosa = c.kind == HIPFEAT_LIBROSA_FBANK;
  if ((c.kind > HIPFEAT_MFCC && !librosa) || route_env("HIPFEAT_FORCE_GENERIC") || route_env("HIPFEAT_NO_WAVE_KERNEL")) return HIPFEAT_OK;
  const int fft = c.fft_length, H = fft / 2;
  // H = 128 (fft 256) stays on the radix-2 kernel: measured 0.92 M vs 0.72 M cuts/s there; H = 256: 0.46 vs 0.48 M
  if (!(fft == 512 || fft == 1024 || fft == 2048) || c.num_filters > 128) return HIPFEAT_OK;
  const WaveTables t = build_wave_tables(in, H);
  const GenericParams& g = std::get<GenericParams>(p->params);  // the window, W_fft^k, DCT matrix and lifter are the generic kernel's
  WaveParams q{};
  q.window = g.window, q.tw = g.tw, q.dct = g.dct, q.lifter = g.lifter;
  hipfeat_status st;
  if (in.M > 0 && (st = upload(p->uploads, q.mel_blob, t.blob.data(), t.blob.size())) != HIPFEAT_OK) return st;
  fill_wave_front(q, c, t);
  q.frames_per_wave = 8;  // 4 waves x 8 frames (the tables copied to LDS per workgroup are ~12 KB)
  q.npad_left = p->npad_left;
  const void* fn = for_n1(H / 64, [](auto n) -> const void* {  // (no instance for n1 = 2: H = 128 was turned away above)
    if constexpr (decltype(n)::value > 2) return entry<wave_kernel<decltype(n)::value>>();
    return nullptr;
  });
  if ((st = claim(p, Route::Wave, fn, 256, t.lds, q)) != HIPFEAT_OK) return st;
  p->kernel_name = strf("wave_kernel<%d> fft=%d lds=%zuB blocks/CU=%d", H / 64, c.fft_length, t.lds, p->blocks_per_cu);
  p->fpb = 4 * q.frames_per_wave;
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// whisper: 400 = 16 x 25 mixed-radix FFT on the vector ALUs.  whisper3 (kernel_whisper3.hpp: wave-autonomous, the normalisation fused)
// when the filterbank schedule and the LDS budget allow, else whisper2 (kernel_whisper2.hpp: banded mel GEMM, normalisation in a
// separate pass); whisper3 reads whisper2's DFT-25 table
// --------------------------------------------------------------------------------------
static hipfeat_status setup_whisper3(hipfeat_plan* p, const PlanInputs& in, const float* d_cs) {
  const WaveAutoTables t = build_whisper3_tables(in, {kW3PRowStride, kW3MaxSets, kW3Steps, kW3Waves, kW3Region}, kW3Span, kW3Tail);
  if (!t.fits || t.lds > 80 * 1024) return HIPFEAT_OK;  // two workgroups of 8 waves per CU or nothing
  const void* fn = t.w_nsets == 2 ? entry<whisper3_kernel<2>>() : entry<whisper3_kernel<3>>();
  Whisper3Params q{};
  if (hipfeat_status bad = fill_wave_autonomous(q, p, t)) return bad;
  q.cs = d_cs;
  // 8 waves x 8 rounds x 4 frames = 256 frames per workgroup
  return claim_wave_auto(p, Route::Whisper3, fn, t, q, 4, 8, 16, strf("whisper3_kernel<%d> fft400=16x25 fused-norm", t.w_nsets));
}

static hipfeat_status setup_whisper(hipfeat_plan* p, const PlanInputs& in) {
  const hipfeat_config& c = p->cfg;
  if (c.kind != HIPFEAT_WHISPER || c.frame_length != kW2N || c.frame_shift != kW2Shift || c.num_filters > 16 * kW2MaxMelTiles ||
      route_env("HIPFEAT_FORCE_GENERIC"))
    return HIPFEAT_OK;
  const Whisper2Tables t = build_whisper2_tables(in);
  Whisper2Params q{};
  hipfeat_status st;
  if ((st = upload(p->uploads, q.cs, t.cs.data(), t.cs.size())) != HIPFEAT_OK) return st;
  if ((st = upload(p->uploads, q.tw, t.tw.data(), t.tw.size())) != HIPFEAT_OK) return st;
  if ((st = upload(p->uploads, q.mel_a, t.mel.data(), t.mel.size())) != HIPFEAT_OK) return st;
  if ((st = upload(p->uploads, q.sched, t.sched.data(), t.sched.size())) != HIPFEAT_OK) return st;
  const char* v = route_env("HIPFEAT_WHISPER_VARIANT");
  if (!(v && v[0] == '2')) {  // HIPFEAT_WHISPER_VARIANT=2: whisper2 (tests compare the two)
    if ((st = setup_whisper3(p, in, q.cs)) != HIPFEAT_OK || p->route == Route::Whisper3) return st;
  }
  q.window = std::get<GenericParams>(p->params).window;
  q.M = c.num_filters;
  q.mel_floor = c.mel_floor;
  p->fpb = 16 * kW2TilesPerBlock;
  if ((st = claim(p, Route::Whisper2, entry<whisper2_kernel>(), 256, 0, q)) != HIPFEAT_OK) return st;
  p->kernel_name = strf("whisper_kernel2 fft400=16x25 mel_chunks=%d+%d+%d+%d blocks/CU=%d", t.load[0], t.load[1], t.load[2], t.load[3], p->blocks_per_cu);
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// fft2048 wave-autonomous fbank kernel (kernel_fft2048c.hpp): 44.1 / 48 kHz Kaldi filterbanks, librosa-style log-mel with n_fft 2048
// --------------------------------------------------------------------------------------
static hipfeat_status setup_fft2048c(hipfeat_plan* p, const PlanInputs& in) {
  const hipfeat_config& c = p->cfg;
  const int N = in.N, shift = in.shift;
  const bool librosa = c.kind == HIPFEAT_LIBROSA_FBANK;  // centred frames, |X| or |X|^2, log10 (librosa_fbank.py:66-137)
  if ((c.kind != HIPFEAT_FBANK && !librosa) || c.fft_length != 2048 || N <= 1024 || c.use_energy ||
      (c.use_fft_mag && !librosa) || route_env("HIPFEAT_FORCE_GENERIC") || route_env("HIPFEAT_NO_WAVE_AUTONOMOUS"))
    return HIPFEAT_OK;
  const bool odd = (shift & 1) != 0;
  const int need = (N + 63) / 64;
  const int nrows = odd ? (need <= 18 ? 18 : 32) : (need <= 19 ? 19 : 32);
  // instance with the mel schedule and the frame geometry as compile-time constants (kernel_fft2048c.hpp): the 80-filter Kaldi default at
  // 44.1 / 48 kHz, if the schedule turns out to be 52 + 28 + 16 steps.  The 44.1 kHz one runs 12 waves per workgroup (3 waves/SIMD) without a
  // span prefetch, the span buffer aliasing the exchange / power region (at 48 kHz that layout measured 3 % slower than 8 waves with the prefetch)
  static const int kFixedSteps[3] = {52, 28, 16};
  const bool want = (odd ? nrows == 18 : nrows == 19) && !librosa && !c.use_fft_mag && in.M == 80 &&
                    (odd ? (N == 1102 && shift == 441) : (N == 1200 && shift == 480)) && !c.snip_edges && !route_env("HIPFEAT_NO_FIXED_SCHEDULE");
  // (HIPFEAT_FFT2048_W12 = 1 / 0: routing switch, forces / forbids the 12-wave layout for either default -- same-call A/Bs)
  const char* w12_env = route_env("HIPFEAT_FFT2048_W12");
  const WaveAutoTables t = build_fft2048c_tables(in, nrows, {kXPRowStride, kXMaxSets, kXMaxSteps, kXMaxWaves, kXRegion}, kXSplitSteps, kXWavesFixed,
                                                 want ? kFixedSteps : nullptr, w12_env ? w12_env[0] == '1' : odd, 160 * 1024);
  if (!t.fits || (t.xs_floats >> 8) > 10 || t.waves < 4) return HIPFEAT_OK;
  if (t.fixed && t.waves != (t.w12 ? kXWavesFixed : kXMaxWaves)) return HIPFEAT_OK;  // (cannot happen for the default geometry: its LDS image fits)
  const void* fn = t.fixed ? (odd ? (t.w12 ? entry<fft2048c_kernel<18, true, 52, 28, 16, true>>() : entry<fft2048c_kernel<18, true, 52, 28, 16>>())
                                  : (t.w12 ? entry<fft2048c_kernel<19, false, 52, 28, 16, true>>() : entry<fft2048c_kernel<19, false, 52, 28, 16>>()))
                   : odd ? (nrows == 18 ? entry<fft2048c_kernel<18, true>>() : entry<fft2048c_kernel<32, true>>())
                         : (nrows == 19 ? entry<fft2048c_kernel<19, false>>() : entry<fft2048c_kernel<32, false>>());
  Fft2048cParams q{};
  hipfeat_status st = fill_wave_autonomous(q, p, t);
  if (st == HIPFEAT_OK && !t.twp.empty()) st = upload(p->uploads, q.twp, t.twp.data(), t.twp.size());
  if (st != HIPFEAT_OK) return st;
  fill_frames(q, p, t);
  fill_sets(q, t);
  q.waves = t.waves;
  q.tws_off = t.tws_off;
  q.tw32_off = t.tw32_off;
  return claim_wave_auto(p, Route::Fft2048c, fn, t, q, 2, 8, 64,
                         strf("fft2048c_kernel<%d,%d> fbank%s waves=%d", nrows, (int)odd, t.fixed ? " fixed-schedule" : "", t.waves));
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_plan_create(const hipfeat_config* cfg, const float* h_window,
                                              const float* h_mel, const float* h_dct, const float* h_lifter,
                                              int32_t device, hipfeat_plan** out) {
  if (!cfg || !out) return fail(HIPFEAT_ERR_INVALID, "cfg/plan pointer is NULL");
  *out = nullptr;
  if (hipfeat_status bad = check_feature_config(cfg, h_window, h_mel, h_dct, h_lifter)) return bad;
  const int N = cfg->frame_length, shift = cfg->frame_shift, fft = cfg->fft_length;
  const bool whisper = cfg->kind == HIPFEAT_WHISPER;
  if (whisper && (fft != N || cfg->snip_edges || cfg->use_energy || cfg->use_fft_mag || cfg->remove_dc_offset || cfg->preemph_coeff != 0.0f))
    return fail(HIPFEAT_ERR_INVALID, "whisper: needs fft_length == frame_length and no snip_edges / energy / magnitude / DC removal / pre-emphasis");
  const bool librosa = cfg->kind == HIPFEAT_LIBROSA_FBANK;
  if (librosa && (cfg->snip_edges || cfg->use_energy))
    return fail(HIPFEAT_ERR_INVALID, "librosa fbank: snip_edges / use_energy are not defined");
  if ((whisper || librosa) && (cfg->num_filters <= 0 || !h_mel)) return fail(HIPFEAT_ERR_INVALID, kNeedMel);
  if (fft > 8192) return fail(HIPFEAT_ERR_UNSUPPORTED, "fft_length %d > 8192 is not supported", fft);
  const bool need_mel = cfg->kind >= HIPFEAT_FBANK;

  hipfeat_plan* p = new (std::nothrow) hipfeat_plan();
  if (!p) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  p->cfg = *cfg;
  p->device = device;
  const int K = fft / 2 + 1;
  const bool pow2 = (fft & (fft - 1)) == 0 && fft >= 2;
  const int H = pow2 ? fft / 2 : 0;
  p->npad_left = (whisper || librosa) ? N / 2 : (cfg->snip_edges ? 0 : (N - shift) / 2);
  const int M = need_mel ? cfg->num_filters : 0;
  const int C = cfg->kind == HIPFEAT_MFCC ? cfg->num_ceps : 0;
  p->feature_dim = feature_dim(*cfg);

  if (hipfeat_status bad = require_gfx950(device)) {
    delete p;
    return bad;
  }
  DeviceGuard g(device);
  hipfeat_status st = HIPFEAT_OK;
  auto bail = [&](hipfeat_status s) {
    plan_free(p);
    return s;
  };

  // the generic kernel's Params: they stay unless a specialised kernel claims the plan, and the setups read the tables they share from them
  GenericParams& gp = std::get<GenericParams>(p->params);
  const std::vector<float2> tw = fft_twiddles(fft, pow2 ? H : fft);
  if ((st = upload(p->uploads, gp.tw, tw.data(), tw.size())) != HIPFEAT_OK) return bail(st);
  if ((st = upload(p->uploads, gp.window, h_window, (size_t)N)) != HIPFEAT_OK) return bail(st);
  if (need_mel) {
    if ((st = upload(p->uploads, gp.mel, h_mel, (size_t)K * M)) != HIPFEAT_OK) return bail(st);
    std::vector<int2> rng(M);  // band of each filter: [first non-zero bin, last non-zero bin + 1)
    for (int j = 0; j < M; ++j) {
      const MelBand b = mel_band(h_mel, M, K, j, j + 1);
      rng[j] = make_int2(b.lo, b.hi);
    }
    if ((st = upload(p->uploads, gp.mel_range, rng.data(), rng.size())) != HIPFEAT_OK) return bail(st);
  }
  if (C) {
    if ((st = upload(p->uploads, gp.dct, h_dct, (size_t)M * C)) != HIPFEAT_OK) return bail(st);
    if (cfg->apply_lifter && (st = upload(p->uploads, gp.lifter, h_lifter, (size_t)C)) != HIPFEAT_OK) return bail(st);
  }

  // LDS carve-up of the generic kernel.  Frames per workgroup: the largest of 8/4/2 whose footprint stays <= 21 KB
  // (7-8 workgroups = full wave occupancy per CU); large FFTs that cannot get there take 2 frames if that fits 64 KB,
  // else 1.  Measured on MI355X (cuts/s of 10 s cuts): fft 512: 8 -> 4 frames 373 k -> 458 k; fft 1024: 8 -> 2 frames
  // 117 k -> 209 k; fft 2048: 8 -> 2 frames 30 k -> 67 k (1 frame: 59 k).
  auto carve = [&](int fpb) {
    auto al = [](int v) { return (v + 3) & ~3; };
    p->fpb = fpb;
    gp.span = (fpb - 1) * shift + N;
    gp.off_z = al(gp.span);
    gp.off_p = gp.off_z + al(fpb * fft);
    gp.off_tw = gp.off_p + al(fpb * K);
    gp.off_stat = gp.off_tw + (pow2 ? al(2 * std::max(H, 1)) : 0);
    gp.off_mel = gp.off_stat + al(2 * fpb);
    const int end = gp.off_mel + al(fpb * std::max(M, 1));
    p->lds = (size_t)end * sizeof(float);
    return p->lds;
  };
  {
    size_t cap = 21 * 1024;
    int pick = 0;
    for (int fpb = 8; fpb >= 2 && !pick; fpb >>= 1)
      if (carve(fpb) <= cap) pick = fpb;
    if (!pick) pick = carve(2) <= 64 * 1024 ? 2 : 1;
    if (carve(pick) > 160 * 1024) p->fpb = 0;
  }
  if (p->fpb < 1) return bail(fail(HIPFEAT_ERR_UNSUPPORTED, "configuration does not fit in LDS"));
  gp.N = N;
  gp.shift = shift;
  gp.fft = fft;
  gp.H = H;
  while (pow2 && (1 << gp.log2H) < H) ++gp.log2H;
  gp.K = K;
  gp.M = cfg->num_filters;
  gp.C = cfg->num_ceps;
  gp.kind = (whisper || librosa) ? (int)HIPFEAT_FBANK : cfg->kind;  // same epilogue with log10; Whisper: launch()'s post-pass finishes it
  gp.flags = energy_flags(*cfg) | (pow2 ? F_POW2 : 0) | ((whisper || librosa) ? (F_CENTER | F_LOG10) : 0);
  gp.fpb = p->fpb;
  gp.npad_left = p->npad_left;
  gp.preemph = cfg->preemph_coeff;
  gp.log_energy_floor = log_energy_floor(cfg->energy_floor);
  gp.mel_floor = cfg->mel_floor;
  gp.log_offset = cfg->log_offset;
  // ... and its launch
  p->fn = reinterpret_cast<const void*>(&generic_kernel);
  p->block = 256;
  if ((st = set_dynamic_lds(p->fn, p->lds)) != HIPFEAT_OK) return bail(st);

  // the specialised kernels, in order of preference: the first setup that claims the plan ends the search
  auto unclaimed = [&](hipfeat_status s) {
    st = s;
    return st == HIPFEAT_OK && p->route == Route::Generic;
  };
  PlanInputs in;
  in.N = N, in.shift = shift, in.K = K, in.M = M, in.C = C;
  in.window = h_window, in.mel = h_mel, in.dct = h_dct, in.lifter = cfg->apply_lifter ? h_lifter : nullptr;
  if (unclaimed(setup_fft512(p, in)) && unclaimed(setup_whisper(p, in)) && unclaimed(setup_fft256(p, in)) && unclaimed(setup_fft1024c(p, in)) &&
      unclaimed(setup_fft2048c(p, in)))
    st = setup_wave(p, in);
  if (st != HIPFEAT_OK) return bail(st);

  *out = p;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_plan_destroy(hipfeat_plan* plan) {
  plan_free(plan);
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API int32_t hipfeat_plan_feature_dim(const hipfeat_plan* plan) { return plan ? plan->feature_dim : 0; }
extern "C" HIPFEAT_API const char* hipfeat_plan_kernel_name(const hipfeat_plan* plan) { return plan ? plan->kernel_name.c_str() : ""; }

// --------------------------------------------------------------------------------------
// layout
// --------------------------------------------------------------------------------------
// Validates the batch and fills the host-side descriptor table.
static hipfeat_status build_descs(const hipfeat_plan* plan, int64_t batch, const int64_t* offs, const int64_t* ns,
                                  const int64_t* padded, const int64_t* out_rows, int64_t out_row_stride,
                                  std::vector<CutDesc>& descs, hipfeat_layout* lay) {
  if (!plan) return fail(HIPFEAT_ERR_INVALID, "plan is NULL");
  if (batch < 0 || (batch > 0 && (!offs || !ns))) return fail(HIPFEAT_ERR_INVALID, "bad batch arguments");
  if (out_row_stride < plan->feature_dim)
    return fail(HIPFEAT_ERR_INVALID, "out_row_stride %lld < feature_dim %d", (long long)out_row_stride, plan->feature_dim);
  const hipfeat_config& c = plan->cfg;
  descs.resize((size_t)batch);
  lay->num_frames.resize((size_t)batch);
  int64_t row = 0, blocks = 0;
  int uniform = -1;
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t S = ns[b], P = padded ? padded[b] : ns[b];
    if (S < 0 || P < S || P > INT32_MAX)
      return fail(HIPFEAT_ERR_INVALID, "cut %lld: num_samples=%lld padded_len=%lld out of range", (long long)b, (long long)S, (long long)P);
    int64_t T = hipfeat_num_frames(S, c.frame_length, c.frame_shift, c.snip_edges);
    if (c.kind == HIPFEAT_WHISPER || c.kind == HIPFEAT_LIBROSA_FBANK) {
      if (P != S) return fail(HIPFEAT_ERR_INVALID, "centred framing: zero-padded batch rows (padded_len != num_samples) are not defined");
      if (S <= c.frame_length / 2)  // torch.stft: reflect padding must be shorter than the signal
        return fail(HIPFEAT_ERR_TOO_SHORT, "cut %lld: %lld samples are not longer than the reflect padding (%d)", (long long)b, (long long)S,
                    c.frame_length / 2);
    } else if (padded) {
      // _extract_batch (extractors.py:499-537): the padded row of P samples is framed as a whole and
      // item b keeps the first compute_num_frames_from_samples(S) rows (lhotse/utils.py:424-434) --
      // with snip_edges that is NOT the snip_edges count, and it is capped by what the row yields.
      const int64_t hop = c.batch_hop > 0 ? c.batch_hop : c.frame_shift;
      T = std::min<int64_t>((S + hop / 2) / hop, hipfeat_num_frames(P, c.frame_length, c.frame_shift, c.snip_edges));
    }
    if (!c.snip_edges && T > 0 && c.kind != HIPFEAT_WHISPER && c.kind != HIPFEAT_LIBROSA_FBANK) {
      hipfeat_status st = hipfeat_check_length(P, c.frame_length, c.frame_shift, 0);
      if (st != HIPFEAT_OK) return st;
    }
    if (!c.snip_edges && T == 0)
      return fail(HIPFEAT_ERR_TOO_SHORT, "cut %lld: %lld samples yield no frames", (long long)b, (long long)S);
    CutDesc& d = descs[(size_t)b];
    d.wave_off = offs[b];
    d.out_row = out_rows ? out_rows[b] : row;
    d.num_samples = (int32_t)S;
    d.padded_len = (int32_t)P;
    d.num_frames = (int32_t)T;
    row += T;
    lay->num_frames[(size_t)b] = T;
  }
  // frames per workgroup: fixed by the plan, or (wave-autonomous kernels) rounds x fpb_unit with the rounds that minimise
  // waves x (start-up + rounds) for this batch (layout_rounds.hpp; round 3's rule: the largest power of two that still gave four waves,
  // else 2)
  int fpb = plan->fpb;
  if (plan->fpb_unit > 0) {
    static const int forced = exp_env("HIPFEAT_ROUNDS") ? atoi(exp_env("HIPFEAT_ROUNDS")) : 0;
    static const bool old_rule = exp_env("HIPFEAT_ROUNDS_R3") != nullptr;
    int rounds = plan->c_rounds_max;
    if (forced >= 1 && forced <= plan->c_rounds_max) {
      rounds = forced;
    } else if (old_rule) {
      for (; rounds > 2; rounds >>= 1)
        if (layout_workgroups_per_cut(lay->num_frames.data(), batch, plan->fpb_unit, rounds, 1) >= 4 * layout_slots(plan->blocks_per_cu)) break;
    } else {
      rounds = layout_rounds_per_cut(lay->num_frames.data(), batch, plan->fpb_unit, plan->c_rounds_max, plan->blocks_per_cu);
    }
    fpb = plan->fpb_unit * rounds;
  }
  // Ragged batch on the 16 kHz default kernel: laid out by frame quads instead of by cuts (kernel_fft512c.hpp, FLAT) -- no half-empty last
  // workgroup per cut, long workgroups whatever the cuts' lengths
  bool ragged = false;
  for (int64_t b = 1; b < batch && !ragged; ++b) ragged = lay->num_frames[(size_t)b] != lay->num_frames[0];
  static const bool no_flat = route_env("HIPFEAT_NO_FLAT") != nullptr;
  lay->flat = ragged && !no_flat && plan->fn_flat;
  lay->total_quads = 0;
  lay->block_cut.clear();
  if (lay->flat) {
    int64_t quads = 0;
    for (int64_t b = 0; b < batch; ++b) {
      if (quads > INT32_MAX - (1 << 24)) return fail(HIPFEAT_ERR_INVALID, "batch too large for one launch");
      descs[(size_t)b].first_block = (int32_t)quads;
      quads += (lay->num_frames[(size_t)b] + 3) / 4;
    }
    static const int forced = exp_env("HIPFEAT_ROUNDS") ? atoi(exp_env("HIPFEAT_ROUNDS")) : 0;
    const int waves_per_wg = plan->fpb_unit / 4;  // a wave takes one quad per round
    const int rounds = forced >= 1 && forced <= plan->c_rounds_max ? forced
                                                                   : layout_rounds_quads(quads, plan->fpb_unit, plan->c_rounds_max, plan->blocks_per_cu);
    fpb = plan->fpb_unit * rounds;
    const int64_t qpw = (int64_t)waves_per_wg * rounds;
    blocks = (quads + qpw - 1) / qpw;
    lay->total_quads = quads;
    lay->block_cut.resize((size_t)blocks);
    int64_t cutp = 0;
    for (int64_t g = 0; g < blocks; ++g) {  // the cut that holds a workgroup's first quad
      const int64_t q = g * qpw;
      while (cutp + 1 < batch && descs[(size_t)cutp + 1].first_block <= q) ++cutp;
      lay->block_cut[(size_t)g] = (int32_t)cutp;
    }
    uniform = 0;
  } else {
    for (int64_t b = 0; b < batch; ++b) {
      if (blocks > INT32_MAX - (1 << 24)) return fail(HIPFEAT_ERR_INVALID, "batch too large for one launch");
      descs[(size_t)b].first_block = (int32_t)blocks;
      const int64_t nb = (lay->num_frames[(size_t)b] + fpb - 1) / fpb;
      blocks += nb;
      if (uniform == -1) uniform = (int)nb;
      else if (uniform != (int)nb) uniform = 0;
    }
  }
  lay->batch = batch;
  lay->total_frames = row;
  lay->total_blocks = blocks;
  lay->out_row_stride = out_row_stride;
  lay->uniform_bpc = uniform > 0 ? uniform : -1;  // -1: ragged, the workgroup -> cut map sits behind the descriptor table (common.hpp)
  if (uniform <= 0 && !lay->flat) {
    lay->block_cut.resize((size_t)blocks);
    for (int64_t b = 0; b < batch; ++b) {
      const int64_t b0 = descs[(size_t)b].first_block, b1 = b + 1 < batch ? descs[(size_t)b + 1].first_block : blocks;
      std::fill(lay->block_cut.begin() + b0, lay->block_cut.begin() + b1, (int32_t)b);
    }
  }
  lay->fpb = fpb;
  lay->fpb_unit = plan->fpb_unit;
  lay->device = plan->device;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_layout_create(const hipfeat_plan* plan, int64_t batch, const int64_t* h_wave_offsets,
                                                const int64_t* h_num_samples, const int64_t* h_padded_len,
                                                const int64_t* h_out_rows, int64_t out_row_stride, void* stream,
                                                hipfeat_layout** layout) {
  if (!layout) return fail(HIPFEAT_ERR_INVALID, "layout pointer is NULL");
  *layout = nullptr;
  hipfeat_layout* lay = new (std::nothrow) hipfeat_layout();
  if (!lay) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  std::vector<CutDesc> descs;
  hipfeat_status st = build_descs(plan, batch, h_wave_offsets, h_num_samples, h_padded_len, h_out_rows, out_row_stride, descs, lay);
  if (st != HIPFEAT_OK) {
    delete lay;
    return st;
  }
  DeviceGuard g(plan->device);
  // one allocation: descriptors, then (Whisper with the fused normalisation) kNormSlots armed copies of the normalisation scratch
  // (ragged batches: the workgroup -> cut map directly behind the descriptors, common.hpp::block_cut_map)
  const size_t map_bytes = (lay->block_cut.size() * sizeof(int32_t) + 15) & ~(size_t)15;
  const size_t desc_bytes = std::max<size_t>(descs.size(), 1) * sizeof(CutDesc) + map_bytes;
  const size_t norm_bytes = plan->route == Route::Whisper3 ? (size_t)kNormSlots * norm_slot_bytes(lay) : 0;
  std::vector<unsigned char> blob(desc_bytes + norm_bytes, 0);  // zeros = armed counters
  if (!descs.empty()) std::memcpy(blob.data(), descs.data(), descs.size() * sizeof(CutDesc));
  if (map_bytes) std::memcpy(blob.data() + descs.size() * sizeof(CutDesc), lay->block_cut.data(), lay->block_cut.size() * sizeof(int32_t));
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&lay->d_cuts), blob.size());
  if (e == hipSuccess && !descs.empty()) {
    // synchronous w.r.t. the host (pageable source), ordered on `stream`
    e = hipMemcpyAsync(lay->d_cuts, blob.data(), blob.size(), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  }
  if (norm_bytes) {
    lay->d_norm = reinterpret_cast<unsigned char*>(lay->d_cuts) + desc_bytes;
    lay->norm_slots = kNormSlots;
  }
  if (e != hipSuccess) {
    (void)hipFree(lay->d_cuts);
    delete lay;
    return fail(HIPFEAT_ERR_HIP, "layout upload failed: %s", hipGetErrorName(e));
  }
  *layout = lay;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_layout_destroy(hipfeat_layout* layout) {
  if (!layout) return HIPFEAT_OK;
  if (layout->owns && layout->d_cuts) {
    DeviceGuard g(layout->device);
    (void)hipFree(layout->d_cuts);
  }
  delete layout;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API int64_t hipfeat_layout_total_frames(const hipfeat_layout* layout) { return layout ? layout->total_frames : 0; }

extern "C" HIPFEAT_API hipfeat_status hipfeat_layout_num_frames(const hipfeat_layout* layout, int64_t* h_num_frames) {
  if (!layout || !h_num_frames) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::copy(layout->num_frames.begin(), layout->num_frames.end(), h_num_frames);
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// launch
// --------------------------------------------------------------------------------------
template <typename P>
constexpr bool kWaveAutonomous = std::is_same_v<P, Whisper3Params> || std::is_same_v<P, Fft512cParams> || std::is_same_v<P, Fft1024cParams> || std::is_same_v<P, Fft2048cParams>;

// What a launch binds in its copy of the plan's Params: the buffers and the layout, in the fields the family has
template <typename P>
static void bind_launch(P& p, const hipfeat_plan* plan, const hipfeat_layout* lay, const float* d_wave, float* d_out) {
  p.wave = d_wave;
  p.out = d_out;
  p.cuts = lay->d_cuts;
  p.out_stride = lay->out_row_stride;
  p.num_cuts = (int32_t)lay->batch;
  p.uniform_bpc = lay->uniform_bpc;
  if constexpr (kWaveAutonomous<P>) {  // workgroups of the layout's rounds of frames
    p.frames_per_block = lay->fpb;
    p.rounds = lay->fpb / plan->fpb_unit;
  }
  if constexpr (std::is_same_v<P, Fft512cParams>) {
    if (plan->route == Route::Fft512c) p.total_quads = (int32_t)lay->total_quads;
  }
  if constexpr (std::is_same_v<P, Whisper3Params>) {
    p.total_blocks = (int32_t)lay->total_blocks;
    if (lay->d_norm) {
      unsigned char* slot = lay->d_norm + (size_t)(lay->norm_next.fetch_add(1u) % (unsigned)lay->norm_slots) * norm_slot_bytes(lay);
      p.wg_stat = reinterpret_cast<float*>(slot);
      p.cut_done = reinterpret_cast<uint32_t*>(slot + 2 * (size_t)lay->total_blocks * sizeof(float));
    }
  }
}

static hipfeat_status launch(const hipfeat_plan* plan, const hipfeat_layout* lay, const float* d_wave, float* d_out,
                             hipStream_t stream) {
  if (lay->total_blocks == 0) return HIPFEAT_OK;
  if (!d_wave || !d_out) return fail(HIPFEAT_ERR_INVALID, "wave/out pointer is NULL");
  if ((plan->fpb_unit > 0 ? (lay->fpb_unit != plan->fpb_unit || lay->fpb % plan->fpb_unit != 0) : lay->fpb != plan->fpb) || lay->device != plan->device)
    return fail(HIPFEAT_ERR_INVALID, "layout was created for a different plan");
  const hipfeat_config& c = plan->cfg;
  const bool whisper = c.kind == HIPFEAT_WHISPER;
  // the kernel's one argument: a copy of the plan's Params with this call bound
  KernelParams params = plan->params;
  void* arg = std::visit(
      [&](auto& p) -> void* {
        bind_launch(p, plan, lay, d_wave, d_out);
        return &p;
      },
      params);
  const bool far = plan->fn_far && lay->out_row_stride >= kMel4WideMaxStride;
  const void* fn = lay->flat && plan->fn_flat ? (far ? plan->fn_flat_far : plan->fn_flat) : (far ? plan->fn_far : plan->fn);
  void* args[] = {arg};
  DeviceGuard g(plan->device);
  set_lds_poison(plan->lds);
  (void)hipLaunchKernel(fn, dim3((unsigned)lay->total_blocks), dim3(plan->block), args, plan->lds, stream);
  HIP_TRY(hipGetLastError());
  // Whisper: the normalisation pass over every cut, unless whisper3 fused it (then the layout carries the scratch)
  if (whisper && !(plan->route == Route::Whisper3 && lay->d_norm)) {
    hipLaunchKernelGGL(whisper_norm_kernel, dim3((unsigned)lay->batch), dim3(1024), 0, stream, lay->d_cuts, d_out, lay->out_row_stride,
                       (int32_t)c.num_filters, (int32_t)c.frame_shift);
    HIP_TRY(hipGetLastError());
  }
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_extract_layout(const hipfeat_plan* plan, const hipfeat_layout* layout,
                                                 const float* d_wave, float* d_out, void* stream) {
  if (!plan || !layout) return fail(HIPFEAT_ERR_INVALID, "plan/layout is NULL");
  return launch(plan, layout, d_wave, d_out, (hipStream_t)stream);
}

// fills rows [num_frames, rows_per_cut) of every cut's slot in a collated (B, rows_per_cut, F) output
__global__ __launch_bounds__(256) void fill_padding_kernel(const CutDesc* __restrict__ cuts, float* __restrict__ out, int64_t row_stride,
                                                           int32_t rows_per_cut, int32_t feature_dim, float value) {
  const CutDesc cd = cuts[blockIdx.y];
  const int64_t n = (int64_t)(rows_per_cut - cd.num_frames) * feature_dim;
  float* __restrict__ base = out + (cd.out_row + cd.num_frames) * row_stride;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / feature_dim;
    base[r * row_stride + (i - r * feature_dim)] = value;
  }
}

__global__ __launch_bounds__(256) void pcm16_to_float_kernel(const int16_t* __restrict__ in, float* __restrict__ out, int64_t n) {
  // 8 samples per lane per step: one 16-byte load, two 16-byte stores
  const int64_t n8 = n >> 3;
  const bool aligned = ((reinterpret_cast<uintptr_t>(in) & 15) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  constexpr float k = 1.0f / 32768.0f;
  if (aligned) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
      const int4 v = reinterpret_cast<const int4*>(in)[i];
      const int w[4] = {v.x, v.y, v.z, v.w};
      float4 a, b;
      a.x = (float)(int16_t)(w[0] & 0xffff) * k; a.y = (float)(w[0] >> 16) * k;
      a.z = (float)(int16_t)(w[1] & 0xffff) * k; a.w = (float)(w[1] >> 16) * k;
      b.x = (float)(int16_t)(w[2] & 0xffff) * k; b.y = (float)(w[2] >> 16) * k;
      b.z = (float)(int16_t)(w[3] & 0xffff) * k; b.w = (float)(w[3] >> 16) * k;
      reinterpret_cast<float4*>(out)[2 * i] = a;
      reinterpret_cast<float4*>(out)[2 * i + 1] = b;
    }
    for (int64_t i = (n8 << 3) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = (float)in[i] * k;
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = (float)in[i] * k;
  }
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_pcm16_to_float(const int16_t* d_pcm, float* d_wave, int64_t num_samples, void* stream) {
  if (num_samples < 0 || (num_samples > 0 && (!d_pcm || !d_wave))) return fail(HIPFEAT_ERR_INVALID, "bad pcm16 arguments");
  if (num_samples == 0) return HIPFEAT_OK;
  const int64_t blocks = std::min<int64_t>((num_samples / 8 + 255) / 256 + 1, 256 * 32);
  hipLaunchKernelGGL(pcm16_to_float_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_pcm, d_wave, num_samples);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HIPFEAT_ERR_HIP, "pcm16 launch failed: %s", hipGetErrorName(e));
  return HIPFEAT_OK;
}

__global__ __launch_bounds__(256) void float_to_half_kernel(const float* __restrict__ in, uint16_t* __restrict__ out, int64_t n) {
  // 8 values per lane per step (two 16-byte loads, one 16-byte store) when both buffers are 16-byte aligned; v_cvt_pkrtz would round
  // towards zero, so the conversion is the scalar round-to-nearest-even one
  const int64_t n8 = n >> 3;
  const bool aligned = ((reinterpret_cast<uintptr_t>(in) & 15) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
  auto cvt = [](float x) -> unsigned { return (unsigned)__builtin_bit_cast(unsigned short, (_Float16)x); };
  if (aligned) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
      const float4 a = reinterpret_cast<const float4*>(in)[2 * i], b = reinterpret_cast<const float4*>(in)[2 * i + 1];
      uint4 o;
      o.x = cvt(a.x) | (cvt(a.y) << 16);
      o.y = cvt(a.z) | (cvt(a.w) << 16);
      o.z = cvt(b.x) | (cvt(b.y) << 16);
      o.w = cvt(b.z) | (cvt(b.w) << 16);
      reinterpret_cast<uint4*>(out)[i] = o;
    }
    for (int64_t i = (n8 << 3) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = (uint16_t)cvt(in[i]);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = (uint16_t)cvt(in[i]);
  }
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_float_to_half(const float* d_in, uint16_t* d_out, int64_t n, void* stream) {
  if (n < 0 || (n > 0 && (!d_in || !d_out))) return fail(HIPFEAT_ERR_INVALID, "bad float_to_half arguments");
  if (n == 0) return HIPFEAT_OK;
  const int64_t blocks = std::min<int64_t>((n / 8 + 255) / 256 + 1, 256 * 32);
  hipLaunchKernelGGL(float_to_half_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_in, d_out, n);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HIPFEAT_ERR_HIP, "float_to_half launch failed: %s", hipGetErrorName(e));
  return HIPFEAT_OK;
}

// transient layout: descriptors staged through a pinned ring slot so the call stays asynchronous
static hipfeat_status extract_transient(const hipfeat_plan* plan, const float* d_wave, const int64_t* h_wave_offsets,
                                        const int64_t* h_num_samples, const int64_t* h_padded_len, int64_t batch, float* d_out,
                                        const int64_t* h_out_rows, int64_t out_row_stride, void* stream, int64_t rows_per_cut,
                                        float pad_value, int64_t* h_num_frames) {
  if (!plan) return fail(HIPFEAT_ERR_INVALID, "plan is NULL");
  hipfeat_layout lay;
  lay.owns = false;
  std::vector<CutDesc> descs;
  hipfeat_status st = build_descs(plan, batch, h_wave_offsets, h_num_samples, h_padded_len, h_out_rows, out_row_stride, descs, &lay);
  if (st != HIPFEAT_OK) return st;
  int64_t max_pad = 0;
  if (rows_per_cut >= 0) {
    for (int64_t b = 0; b < batch; ++b) {
      if (lay.num_frames[(size_t)b] > rows_per_cut)
        return fail(HIPFEAT_ERR_INVALID, "cut %lld has %lld frames but the collated output holds %lld rows per cut", (long long)b,
                    (long long)lay.num_frames[(size_t)b], (long long)rows_per_cut);
      max_pad = std::max(max_pad, rows_per_cut - lay.num_frames[(size_t)b]);
    }
  }
  if (h_num_frames)
    for (int64_t b = 0; b < batch; ++b) h_num_frames[b] = lay.num_frames[(size_t)b];
  if (lay.total_blocks == 0 && max_pad == 0) return HIPFEAT_OK;
  DeviceGuard g(plan->device);
  // Whisper with the fused normalisation: one armed scratch entry per cut travels behind the descriptors (fresh for every call)
  const size_t map_bytes = (lay.block_cut.size() * sizeof(int32_t) + 15) & ~(size_t)15;  // ragged: workgroup -> cut map behind the descriptors
  const size_t desc_bytes = descs.size() * sizeof(CutDesc) + map_bytes;
  const size_t bytes = desc_bytes + (plan->route == Route::Whisper3 ? norm_slot_bytes(&lay) : 0);
  std::lock_guard<std::mutex> lk(plan->mu);
  StagedSlot& s = plan->ring.take();
  HIP_TRY(stage(s, bytes, bytes, (hipStream_t)stream, [&](unsigned char* h) {
    std::memcpy(h, descs.data(), descs.size() * sizeof(CutDesc));
    if (map_bytes) std::memcpy(h + descs.size() * sizeof(CutDesc), lay.block_cut.data(), lay.block_cut.size() * sizeof(int32_t));
    std::memset(h + desc_bytes, 0, bytes - desc_bytes);
  }));
  lay.d_cuts = static_cast<CutDesc*>(s.d);
  if (bytes > desc_bytes) {
    lay.d_norm = static_cast<unsigned char*>(s.d) + desc_bytes;
    lay.norm_slots = 1;
  }
  st = HIPFEAT_OK;
  if (lay.total_blocks > 0) st = launch(plan, &lay, d_wave, d_out, (hipStream_t)stream);
  if (st == HIPFEAT_OK && max_pad > 0) {
    const int64_t per_cut = max_pad * plan->feature_dim;
    const unsigned gx = (unsigned)std::min<int64_t>((per_cut + 1023) / 1024, 64);
    hipLaunchKernelGGL(fill_padding_kernel, dim3(gx, (unsigned)batch), dim3(256), 0, (hipStream_t)stream, lay.d_cuts, d_out,
                       out_row_stride, (int32_t)rows_per_cut, (int32_t)plan->feature_dim, pad_value);
    hipError_t e1 = hipGetLastError();
    if (e1 != hipSuccess) st = fail(HIPFEAT_ERR_HIP, "padding fill launch failed: %s", hipGetErrorName(e1));
  }
  if (st != HIPFEAT_OK) {  // the refusal of launch() or of the padding fill stands, with its text
    (void)s.record((hipStream_t)stream);
    return st;
  }
  return finish_launches(s, (hipStream_t)stream, hipSuccess, "extract", kWaitedLaunches);
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_extract(const hipfeat_plan* plan, const float* d_wave, const int64_t* h_wave_offsets,
                                          const int64_t* h_num_samples, const int64_t* h_padded_len, int64_t batch,
                                          float* d_out, const int64_t* h_out_rows, int64_t out_row_stride, void* stream) {
  return extract_transient(plan, d_wave, h_wave_offsets, h_num_samples, h_padded_len, batch, d_out, h_out_rows, out_row_stride, stream, -1,
                           0.f, nullptr);
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_extract_collated(const hipfeat_plan* plan, const float* d_wave, const int64_t* h_wave_offsets,
                                                   const int64_t* h_num_samples, const int64_t* h_padded_len, int64_t batch,
                                                   float* d_out, int64_t rows_per_cut, float pad_value, int64_t* h_num_frames,
                                                   void* stream) {
  if (!plan) return fail(HIPFEAT_ERR_INVALID, "plan is NULL");
  if (rows_per_cut < 0 || batch < 0 || batch > 65535) return fail(HIPFEAT_ERR_INVALID, "collated output: bad rows_per_cut / batch (max 65535 cuts)");
  std::vector<int64_t> rows((size_t)batch);
  for (int64_t b = 0; b < batch; ++b) rows[(size_t)b] = b * rows_per_cut;
  return extract_transient(plan, d_wave, h_wave_offsets, h_num_samples, h_padded_len, batch, d_out, rows.data(), plan->feature_dim, stream,
                           rows_per_cut, pad_value, h_num_frames);
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_extract_host(const hipfeat_plan* plan, const float* h_wave, int64_t wave_elems,
                                               const int64_t* h_wave_offsets, const int64_t* h_num_samples,
                                               const int64_t* h_padded_len, int64_t batch, float* h_out,
                                               int64_t out_elems, const int64_t* h_out_rows, int64_t out_row_stride,
                                               void* stream) {
  if (!plan) return fail(HIPFEAT_ERR_INVALID, "plan is NULL");
  if (wave_elems < 0 || out_elems < 0 || (wave_elems && !h_wave) || (out_elems && !h_out))
    return fail(HIPFEAT_ERR_INVALID, "bad host buffers");
  for (int64_t b = 0; b < batch; ++b) {
    if (h_wave_offsets[b] < 0 || h_wave_offsets[b] + h_num_samples[b] > wave_elems)
      return fail(HIPFEAT_ERR_INVALID, "cut %lld lies outside the waveform buffer", (long long)b);
  }
  for (int64_t b = 0, row = 0; b < batch; ++b) {
    const hipfeat_config& c = plan->cfg;
    int64_t T = hipfeat_num_frames(h_num_samples[b], c.frame_length, c.frame_shift, c.snip_edges);
    if (h_padded_len) {
      const int64_t hop = c.batch_hop > 0 ? c.batch_hop : c.frame_shift;
      T = std::min<int64_t>((h_num_samples[b] + hop / 2) / hop, hipfeat_num_frames(h_padded_len[b], c.frame_length, c.frame_shift, c.snip_edges));
    }
    const int64_t r0 = h_out_rows ? h_out_rows[b] : row;
    if (r0 < 0 || (T > 0 && ((r0 + T - 1) * out_row_stride + plan->feature_dim) > out_elems))
      return fail(HIPFEAT_ERR_INVALID, "cut %lld: output rows lie outside the output buffer", (long long)b);
    row += T;
  }
  DeviceGuard g(plan->device);
  hipStream_t st_ = (hipStream_t)stream;
  float *dw, *dout;
  {
    std::lock_guard<std::mutex> lk(plan->mu);
    if (plan->scratch_wave_cap < (size_t)wave_elems) {
      (void)hipFree(plan->d_scratch_wave);
      plan->d_scratch_wave = nullptr;
      plan->scratch_wave_cap = 0;
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&plan->d_scratch_wave), std::max<size_t>(wave_elems, 1) * sizeof(float)));
      plan->scratch_wave_cap = (size_t)wave_elems;
    }
    if (plan->scratch_out_cap < (size_t)out_elems) {
      (void)hipFree(plan->d_scratch_out);
      plan->d_scratch_out = nullptr;
      plan->scratch_out_cap = 0;
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&plan->d_scratch_out), std::max<size_t>(out_elems, 1) * sizeof(float)));
      plan->scratch_out_cap = (size_t)out_elems;
    }
    dw = plan->d_scratch_wave;
    dout = plan->d_scratch_out;
  }
  // rows / columns no cut covers come back as zeros
  if (out_elems) HIP_TRY(hipMemsetAsync(dout, 0, (size_t)out_elems * sizeof(float), st_));
  if (wave_elems) HIP_TRY(hipMemcpyAsync(dw, h_wave, (size_t)wave_elems * sizeof(float), hipMemcpyHostToDevice, st_));
  hipfeat_status st = hipfeat_extract(plan, dw, h_wave_offsets, h_num_samples, h_padded_len, batch, dout, h_out_rows,
                                      out_row_stride, stream);
  if (st != HIPFEAT_OK) return st;
  if (out_elems) HIP_TRY(hipMemcpyAsync(h_out, dout, (size_t)out_elems * sizeof(float), hipMemcpyDeviceToHost, st_));
  HIP_TRY(hipStreamSynchronize(st_));
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// post-feature transforms on the collated batch (GlobalMVN, SpecAugment)
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_API hipfeat_status hipfeat_global_mvn(const float* d_in, float* d_out, const float* d_means, const float* d_stds,
                                                         int64_t rows, int64_t feature_dim, int inverse, void* stream) {
  if (rows < 0 || feature_dim <= 0 || feature_dim > INT32_MAX || (rows > 0 && (!d_in || !d_out)) || !d_means || !d_stds)
    return fail(HIPFEAT_ERR_INVALID, "bad global_mvn arguments");
  const int64_t n = rows * feature_dim;
  if (n == 0) return HIPFEAT_OK;
  const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(global_mvn_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_in, d_out, d_means, d_stds, n,
                     (int32_t)feature_dim, (int32_t)(inverse != 0));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HIPFEAT_ERR_HIP, "global_mvn launch failed: %s", hipGetErrorName(e));
  return HIPFEAT_OK;
}

namespace {
struct StagingRing {
  std::mutex mu;
  SlotRing<4> ring;
};
StagingRing g_rings[64];  // per device, process lifetime, never freed (descriptors of plan-less calls)
}  // namespace

extern "C" HIPFEAT_API hipfeat_status hipfeat_specaug(const float* d_in, float* d_out, int64_t batch, int64_t num_frames, int64_t feature_dim,
                                                      const hipfeat_warp_segment* h_segments, int64_t num_segments,
                                                      const hipfeat_mask* h_masks, int64_t num_masks, void* stream) {
  if (batch < 0 || num_frames < 0 || feature_dim < 0 || num_segments < 0 || num_masks < 0 || (num_segments && !h_segments) ||
      (num_masks && !h_masks))
    return fail(HIPFEAT_ERR_INVALID, "bad specaug arguments");
  if (batch > 65535 || num_frames > (1 << 24) || feature_dim > 32768)
    return fail(HIPFEAT_ERR_INVALID, "specaug: batch <= 65535, num_frames <= 2^24, feature_dim <= 32768");
  if (batch * num_frames * feature_dim == 0) return HIPFEAT_OK;
  if (!d_in || !d_out || d_in == d_out) return fail(HIPFEAT_ERR_INVALID, "specaug: needs distinct input and output buffers");
  const int B = (int)batch, T = (int)num_frames, F = (int)feature_dim;
  // group by sequence (stable), validate
  std::vector<int32_t> seg_off((size_t)B + 1, 0), mask_off((size_t)B + 1, 0);
  for (int64_t i = 0; i < num_segments; ++i) {
    const hipfeat_warp_segment& g = h_segments[i];
    if (g.sequence < 0 || g.sequence >= B || g.start < 0 || g.num_frames < 2 || g.start + (int64_t)g.num_frames > T || g.center < 1 ||
        g.center >= g.num_frames || g.warped < 1 || g.warped >= g.num_frames)
      return fail(HIPFEAT_ERR_INVALID, "specaug: warp segment %lld is out of range", (long long)i);
    seg_off[(size_t)g.sequence + 1]++;
  }
  for (int64_t i = 0; i < num_masks; ++i) {
    const hipfeat_mask& m = h_masks[i];
    if (m.sequence < 0 || m.sequence >= B || (m.axis != 1 && m.axis != 2) || m.begin < 0 || m.end < m.begin)
      return fail(HIPFEAT_ERR_INVALID, "specaug: mask %lld is out of range", (long long)i);
    mask_off[(size_t)m.sequence + 1]++;
  }
  for (int b = 0; b < B; ++b) {
    seg_off[(size_t)b + 1] += seg_off[(size_t)b];
    mask_off[(size_t)b + 1] += mask_off[(size_t)b];
  }
  std::vector<WarpSeg> segs((size_t)num_segments);
  std::vector<int32_t> masks((size_t)num_masks * 3);
  {
    std::vector<int32_t> cur(seg_off.begin(), seg_off.end() - 1);
    for (int64_t i = 0; i < num_segments; ++i) {
      const hipfeat_warp_segment& g = h_segments[i];
      segs[(size_t)cur[(size_t)g.sequence]++] = WarpSeg{g.sequence, g.start, g.num_frames, g.center, g.warped};
    }
    for (int b = 0; b < B; ++b)  // the reference warps segment after segment: overlapping ones would read each other's output
      for (int i = seg_off[(size_t)b]; i < seg_off[(size_t)b + 1]; ++i)
        for (int j = i + 1; j < seg_off[(size_t)b + 1]; ++j)
          if (segs[(size_t)i].start < segs[(size_t)j].start + segs[(size_t)j].len && segs[(size_t)j].start < segs[(size_t)i].start + segs[(size_t)i].len)
            return fail(HIPFEAT_ERR_INVALID, "specaug: warp segments of sequence %d overlap (apply them in separate calls)", b);
    std::vector<int32_t> mc(mask_off.begin(), mask_off.end() - 1);
    for (int64_t i = 0; i < num_masks; ++i) {
      const hipfeat_mask& m = h_masks[i];
      const size_t k = (size_t)mc[(size_t)m.sequence]++ * 3;
      masks[k] = m.axis;
      masks[k + 1] = m.begin;
      masks[k + 2] = m.end;
    }
  }
  int tile_elems = 8192;
  const int rows_per_tile = std::max(1, std::min(T, tile_elems / std::max(F, 1)));
  const int tiles = (T + rows_per_tile - 1) / rows_per_tile;
  auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
  const size_t o_seg_off = 0, o_mask_off = up16(o_seg_off + seg_off.size() * 4), o_segs = up16(o_mask_off + mask_off.size() * 4),
               o_masks = up16(o_segs + segs.size() * sizeof(WarpSeg)), o_part = up16(o_masks + masks.size() * 4),
               h_bytes = o_part, total = o_part + (size_t)B * tiles * 4;
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(HIPFEAT_ERR_INVALID, "device index %d out of range", dev);
  std::lock_guard<std::mutex> lk(g_rings[dev].mu);
  StagedSlot& sl = g_rings[dev].ring.take();  // device: the tables, then the partial sums
  hipStream_t st_ = (hipStream_t)stream;
  HIP_TRY(stage(sl, total, h_bytes, st_, [&](unsigned char* h) {
    std::memcpy(h + o_seg_off, seg_off.data(), seg_off.size() * 4);
    std::memcpy(h + o_mask_off, mask_off.data(), mask_off.size() * 4);
    if (!segs.empty()) std::memcpy(h + o_segs, segs.data(), segs.size() * sizeof(WarpSeg));
    if (!masks.empty()) std::memcpy(h + o_masks, masks.data(), masks.size() * 4);
  }));
  char* d = static_cast<char*>(sl.d);
  SpecAugParams sp{};
  sp.in = d_in;
  sp.out = d_out;
  sp.B = B;
  sp.T = T;
  sp.F = F;
  sp.seg_off = reinterpret_cast<const int32_t*>(d + o_seg_off);
  sp.mask_off = reinterpret_cast<const int32_t*>(d + o_mask_off);
  sp.segs = reinterpret_cast<const WarpSeg*>(d + o_segs);
  sp.masks = reinterpret_cast<const int32_t*>(d + o_masks);
  sp.partials = reinterpret_cast<float*>(d + o_part);
  sp.tiles = tiles;
  sp.rows_per_tile = rows_per_tile;
  const bool vec4 = F % 4 == 0 && ((reinterpret_cast<uintptr_t>(d_in) | reinterpret_cast<uintptr_t>(d_out)) & 15) == 0;
  if (vec4) hipLaunchKernelGGL(specaug_warp_kernel<4>, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, st_, sp);
  else hipLaunchKernelGGL(specaug_warp_kernel<1>, dim3((unsigned)tiles, (unsigned)B), dim3(256), 0, st_, sp);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && num_masks > 0) {
    hipLaunchKernelGGL(specaug_mask_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(256), (size_t)F + rows_per_tile, st_, sp);
    e = hipGetLastError();
  }
  return finish_launches(sl, st_, e, "specaug", kWaitedLaunches);
}

// --------------------------------------------------------------------------------------
// resampler (speed perturbation)
// --------------------------------------------------------------------------------------
struct hipfeat_resampler {
  int device = 0, orig = 0, nw = 0, kw = 0, width = 0;
  float* d_kernel = nullptr;
  int outs_per_block = 2048, span_floats = 0, kernel_in_lds = 0;
  size_t lds_bytes = 0;
  // fast path (compile-time ratio): transposed bank [kw][newp] + launcher
  float* d_kernel_t = nullptr;
  void (*fast)(const float*, float*, const ResCut*, const float*, int, unsigned, hipStream_t) = nullptr;
  int fast_outs = 0;
  // matrix-core path (many-phase ratios): padded transposed bank [kwp][nwp] + geometry (resample_tables.hpp)
  float* d_kernel_mfma = nullptr;
  ResMfmaGeometry mfma;
  char kernel_name[48] = "resample_generic";
  mutable std::mutex mu;
  mutable SlotRing<4> ring;
};

template <int ORIG, int NEW, int WIDTH>
static void launch_resample_fast(const float* in, float* out, const ResCut* cuts, const float* kt, int num_cuts, unsigned blocks,
                                 hipStream_t stream) {
  hipLaunchKernelGGL((resample_fast_kernel<ORIG, NEW, WIDTH>), dim3(blocks), dim3(256), 0, stream, in, out, cuts, kt, num_cuts);
}

template <int ORIG, int NEW, int WIDTH>
static bool pick_resample_fast(hipfeat_resampler* r) {
  if (r->orig != ORIG || r->nw != NEW || r->width != WIDTH) return false;
  r->fast = &launch_resample_fast<ORIG, NEW, WIDTH>;
  r->fast_outs = ResampleFast<ORIG, NEW, WIDTH>::OUTS;
  std::snprintf(r->kernel_name, sizeof(r->kernel_name), "resample_fast<%d,%d,%d>", ORIG, NEW, WIDTH);
  return true;
}

extern "C" HIPFEAT_API int64_t hipfeat_resampled_length(int64_t num_samples, int32_t orig_freq, int32_t new_freq) {
  if (orig_freq <= 0 || new_freq <= 0 || num_samples < 0) return 0;
  // torch.ceil(torch.as_tensor(new * length / orig)): the quotient is a Python float stored as float32
  const float q = (float)((double)new_freq * (double)num_samples / (double)orig_freq);
  return (int64_t)std::ceil(q);
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_resampler_create(int32_t orig_freq, int32_t new_freq, int32_t width,
                                                               const float* h_kernel, int32_t device, hipfeat_resampler** out) {
  if (!out || !h_kernel) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  *out = nullptr;
  if (orig_freq <= 0 || new_freq <= 0 || width <= 0) return fail(HIPFEAT_ERR_INVALID, "bad resampler geometry");
  if (hipfeat_status bad = check_device(device)) return bad;
  hipfeat_resampler* r = new (std::nothrow) hipfeat_resampler();
  if (!r) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  r->device = device;
  r->orig = orig_freq;
  r->nw = new_freq;
  r->width = width;
  r->kw = 2 * width + orig_freq;
  DeviceGuard g(device);
  auto bail = [&](hipfeat_status s) {
    (void)hipfeat_resampler_destroy(r);
    return s;
  };
  hipfeat_status st = upload(&r->d_kernel, h_kernel, (size_t)r->nw * r->kw);
  if (st != HIPFEAT_OK) return bail(st);
  // speed 0.9 / 1.1 / 0.95 / 1.05 at any rate, and the 1:2, 2:1, 3:1 rate conversions
  const bool generic_only = route_env("HIPFEAT_RESAMPLE_GENERIC");
  const bool fast = !generic_only &&
                    (pick_resample_fast<9, 10, 7>(r) || pick_resample_fast<11, 10, 7>(r) || pick_resample_fast<19, 20, 7>(r) ||
                     pick_resample_fast<21, 20, 7>(r) || pick_resample_fast<1, 2, 7>(r) || pick_resample_fast<2, 1, 13>(r) ||
                     pick_resample_fast<3, 1, 19>(r));
  if (fast) {
    const int newp = (r->nw + 3) & ~3;
    std::vector<float> kt((size_t)r->kw * newp, 0.f);
    for (int ph = 0; ph < r->nw; ++ph)
      for (int i = 0; i < r->kw; ++i) kt[(size_t)i * newp + ph] = h_kernel[(size_t)ph * r->kw + i];
    st = upload(&r->d_kernel_t, kt.data(), kt.size());
    if (st != HIPFEAT_OK) return bail(st);
  } else if (!generic_only && (res_mfma_routed(r->orig, r->nw, r->width) ||
                               (route_env("HIPFEAT_RESAMPLE_MFMA") && r->nw >= kResMfmaTile && res_mfma_geometry(r->orig, r->nw, r->width).fits))) {
    // many phases, odd hop: the matrix-core kernel (measured against the generic one by tools/bench_resample_rates.py, which sets
    // HIPFEAT_RESAMPLE_MFMA=1 to time it on the ratios the rule leaves to the generic kernel as well)
    r->mfma = res_mfma_geometry(r->orig, r->nw, r->width);
    const std::vector<float> kt = res_mfma_bank(h_kernel, r->nw, r->kw, r->mfma.kwp, r->mfma.nwp);
    st = upload(&r->d_kernel_mfma, kt.data(), kt.size());
    if (st != HIPFEAT_OK) return bail(st);
    std::snprintf(r->kernel_name, sizeof(r->kernel_name), "resample_mfma");
  }
  r->kernel_in_lds = ((size_t)r->nw * r->kw <= 8192) ? 1 : 0;
  for (r->outs_per_block = 2048; r->outs_per_block >= 64; r->outs_per_block >>= 1) {
    r->span_floats = (((r->outs_per_block + r->nw - 1) / r->nw + 1) * r->orig + r->kw + 3) & ~3;
    r->lds_bytes = ((size_t)r->span_floats + (r->kernel_in_lds ? (size_t)r->nw * r->kw : 0)) * sizeof(float);
    if (r->lds_bytes <= 64 * 1024) break;
  }
  if (r->outs_per_block < 64) return bail(fail(HIPFEAT_ERR_UNSUPPORTED, "resampling ratio %d/%d needs too much LDS", orig_freq, new_freq));
  *out = r;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_resampler_destroy(hipfeat_resampler* r) {
  if (!r) return HIPFEAT_OK;
  DeviceGuard g(r->device);
  (void)hipFree(r->d_kernel);
  if (r->d_kernel_t) (void)hipFree(r->d_kernel_t);
  if (r->d_kernel_mfma) (void)hipFree(r->d_kernel_mfma);
  r->ring.free_all();  // (waits for the launches that used a slot)
  delete r;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API const char* hipfeat_resampler_kernel_name(const hipfeat_resampler* r) { return r ? r->kernel_name : ""; }

extern "C" HIPFEAT_API hipfeat_status hipfeat_resample(const hipfeat_resampler* r, const float* d_in, const int64_t* h_in_offsets,
                                                       const int64_t* h_num_samples, int64_t batch, float* d_out,
                                                       const int64_t* h_out_offsets, void* stream) {
  if (!r) return fail(HIPFEAT_ERR_INVALID, "resampler is NULL");
  if (batch < 0 || (batch > 0 && (!h_in_offsets || !h_num_samples || !h_out_offsets || !d_in || !d_out)))
    return fail(HIPFEAT_ERR_INVALID, "bad batch arguments");
  std::vector<ResCut> cuts((size_t)batch);
  int64_t blocks = 0;
  const int64_t opb = r->fast ? r->fast_outs : r->d_kernel_mfma ? r->mfma.outs_per_block : r->outs_per_block;
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t L = h_num_samples[b];
    if (L < 0 || L > INT32_MAX / 2) return fail(HIPFEAT_ERR_INVALID, "cut %lld: %lld samples out of range", (long long)b, (long long)L);
    const int64_t ol = hipfeat_resampled_length(L, r->orig, r->nw);
    if (ol > INT32_MAX) return fail(HIPFEAT_ERR_INVALID, "cut %lld: output too long", (long long)b);
    cuts[(size_t)b] = ResCut{h_in_offsets[b], h_out_offsets[b], (int32_t)L, (int32_t)ol, (int32_t)blocks, 0};
    blocks += (ol + opb - 1) / opb;
    if (blocks > INT32_MAX - (1 << 24)) return fail(HIPFEAT_ERR_INVALID, "batch too large for one launch");
  }
  if (blocks == 0) return HIPFEAT_OK;
  DeviceGuard g(r->device);
  const size_t bytes = cuts.size() * sizeof(ResCut);
  std::lock_guard<std::mutex> lk(r->mu);
  StagedSlot& s = r->ring.take();
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(stage(s, bytes, bytes, st, [&](unsigned char* h) { std::memcpy(h, cuts.data(), bytes); }));
  const ResCut* d_cuts = static_cast<const ResCut*>(s.d);
  if (r->fast) {
    r->fast(d_in, d_out, d_cuts, r->d_kernel_t, (int)batch, (unsigned)blocks, st);
  } else if (r->d_kernel_mfma) {
    ResMfmaParams mp{};
    mp.in = d_in;
    mp.out = d_out;
    mp.cuts = d_cuts;
    mp.kt = r->d_kernel_mfma;
    mp.num_cuts = (int32_t)batch;
    mp.orig = r->orig;
    mp.nw = r->nw;
    mp.width = r->width;
    mp.kwp = r->mfma.kwp;
    mp.nwp = r->mfma.nwp;
    mp.span_floats = r->mfma.span_floats;
    const dim3 grid((unsigned)blocks), wg(256);
    if (r->mfma.hop_tiles == 4)
      hipLaunchKernelGGL(resample_mfma_kernel<4>, grid, wg, r->mfma.lds_bytes, st, mp);
    else if (r->mfma.hop_tiles == 2)
      hipLaunchKernelGGL(resample_mfma_kernel<2>, grid, wg, r->mfma.lds_bytes, st, mp);
    else
      hipLaunchKernelGGL(resample_mfma_kernel<1>, grid, wg, r->mfma.lds_bytes, st, mp);
  } else {
    ResampleParams rp{};
    rp.in = d_in;
    rp.out = d_out;
    rp.cuts = d_cuts;
    rp.kernel = r->d_kernel;
    rp.num_cuts = (int32_t)batch;
    rp.orig = r->orig;
    rp.nw = r->nw;
    rp.kw = r->kw;
    rp.width = r->width;
    rp.outs_per_block = r->outs_per_block;
    rp.span_floats = r->span_floats;
    rp.kernel_in_lds = r->kernel_in_lds;
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)blocks), dim3(256), r->lds_bytes, st, rp);
  }
  return finish_launches(s, st, hipGetLastError(), "resample", kWaitedLaunch);
}

// --------------------------------------------------------------------------------------
// What the arena handles share ("Ticketed handles"): the handle with its ticket ring (ticket_slots.hpp) and one StagedSlot per
// ticket, and the grid and table-route rules of the launches that walk a flat item list
// --------------------------------------------------------------------------------------
// Plan hands out a ticket and keeps the validated tables in plans[ticket % kTicketSlots]; run stages them through the slot of the same
// index.  A ticket is released when its launches have been issued (enqueued, or refused by the runtime at launch: the ticket has run), just
// before finish_launches: an argument refusal or a failed allocation leaves it planned.
template <typename Plan>
struct TicketedHandle {
  int device = 0;
  bool allow_inline = true;
  std::mutex mu;
  TicketRing tickets;
  Plan plans[kTicketSlots];
  StagedSlot slots[kTicketSlots];
};
struct hipfeat_mixer : TicketedHandle<MixPlan> {};
struct hipfeat_reverb : TicketedHandle<RvMethodPlan> {
  float2* d_tw = nullptr;  // W_2048^k, k < 1024: uploaded by the first run of a ticket with FFT items
  double2* d_tw64 = nullptr;
};
struct hipfeat_level : TicketedHandle<LvPlan> {};
struct hipfeat_collate : TicketedHandle<CoPlan> {};
struct hipfeat_sinc : TicketedHandle<SincPlan> {};
struct hipfeat_featmix : TicketedHandle<FmPlan> {};

template <typename H>
static hipfeat_status handle_create(int32_t device, H** out, const char* what) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "%s pointer is NULL", what);
  *out = nullptr;
  if (hipfeat_status bad = check_device(device)) return bad;
  H* h = new (std::nothrow) H();
  if (!h) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  h->device = device;
  h->allow_inline = route_env("HIPFEAT_MB_NO_INLINE") == nullptr;
  *out = h;
  return HIPFEAT_OK;
}

template <typename H>
static hipfeat_status handle_destroy(H* h) {
  if (!h) return HIPFEAT_OK;
  DeviceGuard g(h->device);
  for (auto& s : h->slots) s.free_all();
  delete h;
  return HIPFEAT_OK;
}

// under the handle's mutex: the ticket of a new plan (never drop a live plan: its ticket would fail at run)
static hipfeat_status take_ticket(TicketRing& tickets, const char* what_plural, int64_t* ticket) {
  *ticket = tickets.take();
  if (*ticket >= 0) return HIPFEAT_OK;
  return fail(HIPFEAT_ERR_INVALID, "%d planned %s are outstanding: run ticket %lld first", kTicketSlots, what_plural,
              (long long)tickets.ticket[tickets.next_ticket % kTicketSlots]);
}

// under the handle's mutex: the slot of a planned ticket, or -1 with the refusal written
static int find_ticket(const TicketRing& tickets, int64_t ticket, const char* what) {
  const int slot = tickets.slot_of(ticket);
  if (slot < 0) (void)fail(HIPFEAT_ERR_INVALID, "ticket %lld is not a planned %s (at most %d plans may be outstanding)", (long long)ticket, what, kTicketSlots);
  return slot;
}

// a few workgroups per CU take the items round-robin; the grid is the smallest one that gives every workgroup the same number of
// items: ceil(items / ceil(items / slots))
static unsigned items_grid(int64_t items, int64_t slots = 1792) {
  const int64_t per_wg = std::max<int64_t>(1, (items + slots - 1) / slots);
  return (unsigned)std::max<int64_t>(1, (items + per_wg - 1) / per_wg);
}

// where a launch finds its tables: in its kernel arguments, or staged -- and then searched in LDS (dynamic LDS = bytes) or where they are
struct TableRoute {
  bool inl;
  size_t dyn;
};
static TableRoute table_route(bool allow_inline, size_t bytes) {
  return {allow_inline && bytes <= (size_t)kMbInlineBytes, bytes <= (size_t)kMbLdsTableBytes ? bytes : 0};
}

// the tables of `args` to where its route reads them: args.blob, or through the slot's pinned buffer to the front of its device buffer
template <typename Args, typename Fill>
static hipError_t place_tables(Args& args, const TableRoute& r, StagedSlot& s, size_t bytes, hipStream_t st, Fill fill) {
  args.h.tables = r.inl ? nullptr : static_cast<const unsigned char*>(s.d);
  fill(r.inl ? args.blob : static_cast<unsigned char*>(s.h));
  return r.inl ? hipSuccess : hipMemcpyAsync(s.d, s.h, bytes, hipMemcpyHostToDevice, st);
}

// --------------------------------------------------------------------------------------
// on-the-fly mini-batch: mixed-factor speed perturbation + collated extraction in two launches (kernel_minibatch.hpp)
// --------------------------------------------------------------------------------------
constexpr int kMbSlots = 16;
constexpr int kMbMaxResamplers = 8;

struct MbSlot : StagedSlot {  // device: the feature launch's CutDesc table and map, then (staged path) the blob
  int64_t ticket = -1;
  bool planned = false;
  const hipfeat_plan* plan = nullptr;
  hipfeat_layout lay;
  std::vector<CutDesc> descs;
  std::vector<ResCut> res;
  std::vector<int32_t> rows;        // rows per cut of the collated tensor each cut belongs to (grouped plans: fixed at plan time)
  std::vector<int64_t> group_first; // first cut of each group, then batch
  int64_t total_rows = 0;
  std::vector<int32_t> fill_first;  // prefix sum of the cuts' padding items (16 KB each)
  int64_t res_blocks = 0, arena_need = 0, max_frames = 0;  // res_blocks: resampler items (256 hops each) of the whole mini-batch
};

struct hipfeat_speed_bank {
  int device = 0;
  bool device_set = false;  // a bank without resamplers learns its device from the first plan it serves
  int num = 0;
  int kind[kMbMaxResamplers] = {};  // kernel_minibatch.hpp's switch index of resampler i
  int orig[kMbMaxResamplers] = {}, nw[kMbMaxResamplers] = {}, outs[kMbMaxResamplers] = {};
  const float* kt[kMbKinds] = {};
  size_t lds_bytes = 0;
  bool allow_inline = true;
  std::mutex mu;
  MbSlot slots[kMbSlots];
  int64_t next_ticket = 0;
};

extern "C" HIPFEAT_API hipfeat_status hipfeat_speed_bank_create(const hipfeat_resampler* const* resamplers, int32_t num,
                                                                hipfeat_speed_bank** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "bank pointer is NULL");
  *out = nullptr;
  if (num < 0 || num > kMbMaxResamplers || (num > 0 && !resamplers)) return fail(HIPFEAT_ERR_INVALID, "a bank holds 0 ... %d resamplers", kMbMaxResamplers);
  hipfeat_speed_bank* b = new (std::nothrow) hipfeat_speed_bank();
  if (!b) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  static const int ratios[kMbKinds][3] = {{9, 10, 7}, {11, 10, 7}};
  static const size_t lds_floats[kMbKinds] = {ResampleFast<9, 10, 7>::LDS_FLOATS, ResampleFast<11, 10, 7>::LDS_FLOATS};
  static const int outs[kMbKinds] = {ResampleFast<9, 10, 7>::OUTS, ResampleFast<11, 10, 7>::OUTS};
  b->lds_bytes = 16;
  for (int i = 0; i < num; ++i) {
    const hipfeat_resampler* r = resamplers[i];
    int k = -1;
    if (r && r->d_kernel_t)
      for (int j = 0; j < kMbKinds; ++j)
        if (r->orig == ratios[j][0] && r->nw == ratios[j][1] && r->width == ratios[j][2]) k = j;
    if (k < 0 || (i > 0 && r->device != b->device)) {
      const int o = r ? r->orig : 0, n = r ? r->nw : 0;
      delete b;
      return fail(HIPFEAT_ERR_UNSUPPORTED, "resampler %d (%d -> %d) is not one of the compile-time ratios of the mixed launch (9:10, 11:10 = speed 0.9 / 1.1), "
                  "or lives on another device: use hipfeat_resample per factor", i, o, n);
    }
    if (i == 0) {
      b->device = r->device;
      b->device_set = true;
    }
    b->kind[i] = k;
    b->orig[i] = r->orig;
    b->nw[i] = r->nw;
    b->outs[i] = outs[k];
    b->kt[k] = r->d_kernel_t;
    b->lds_bytes = std::max(b->lds_bytes, lds_floats[k] * sizeof(float));
  }
  b->num = num;
  b->allow_inline = route_env("HIPFEAT_MB_NO_INLINE") == nullptr;
  *out = b;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_speed_bank_destroy(hipfeat_speed_bank* b) {
  if (!b) return HIPFEAT_OK;
  if (!b->device_set) {  // never served a plan: no slot was ever allocated, and there is no device to touch
    delete b;
    return HIPFEAT_OK;
  }
  DeviceGuard g(b->device);
  for (auto& s : b->slots) s.free_all();
  delete b;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_minibatch_plan(hipfeat_speed_bank* bank, const hipfeat_plan* plan, int64_t batch,
                                                             const int64_t* h_offsets, const int64_t* h_num_samples,
                                                             const int32_t* h_bank_index, const int64_t* h_max_samples,
                                                             int64_t tail_start, int32_t zero_pad_batch, int64_t num_groups,
                                                             const int64_t* h_group_sizes, int64_t* h_out_offsets,
                                                             int64_t* h_out_num_samples, int64_t* h_num_frames, int64_t* h_group_rows,
                                                             int64_t* h_info) {
  if (!bank || !plan || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (batch <= 0 || !h_offsets || !h_num_samples || batch > 65535) return fail(HIPFEAT_ERR_INVALID, "bad batch arguments (1 ... 65535 cuts)");
  if (plan->route == Route::Whisper3 || plan->cfg.kind == HIPFEAT_WHISPER || plan->cfg.kind == HIPFEAT_LIBROSA_FBANK)
    return fail(HIPFEAT_ERR_UNSUPPORTED, "the mini-batch launch pair serves the Kaldi-style plans (spectrogram / fbank / mfcc)");
  if (num_groups < 0 || (num_groups > 0 && !h_group_sizes)) return fail(HIPFEAT_ERR_INVALID, "bad group arguments");
  std::lock_guard<std::mutex> lk(bank->mu);
  if (!bank->device_set) {  // a bank without resamplers (plain collated extraction): its slots live on the device of the plans it serves
    bank->device = plan->device;
    bank->device_set = true;
  }
  if (plan->device != bank->device) return fail(HIPFEAT_ERR_INVALID, "plan (device %d) and bank (device %d) live on different devices", plan->device, bank->device);
  const int64_t ticket = bank->next_ticket++;
  MbSlot& s = bank->slots[ticket % kMbSlots];
  s.planned = false;
  s.ticket = ticket;
  s.plan = plan;
  s.res.clear();
  s.group_first.assign(1, 0);
  if (num_groups > 0) {
    for (int64_t k = 0; k < num_groups; ++k) {
      if (h_group_sizes[k] <= 0) return fail(HIPFEAT_ERR_INVALID, "group %lld is empty", (long long)k);
      s.group_first.push_back(s.group_first.back() + h_group_sizes[k]);
    }
    if (s.group_first.back() != batch) return fail(HIPFEAT_ERR_INVALID, "the groups hold %lld cuts, the batch %lld", (long long)s.group_first.back(), (long long)batch);
  } else {
    s.group_first.push_back(batch);
  }
  // lengths and places of the perturbed batch: unperturbed cuts stay where they are, the others go to the tail in cut order, each on a
  // 16-byte boundary (the feature kernels fetch spans by LDS-DMA)
  std::vector<int64_t> offs((size_t)batch), lens((size_t)batch), padded;
  int64_t tail = (tail_start + 3) & ~(int64_t)3, blocks = 0, max_len = 0;
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t L = h_num_samples[b];
    const int idx = h_bank_index ? h_bank_index[b] : -1;
    if (L < 0 || L > INT32_MAX / 2) return fail(HIPFEAT_ERR_INVALID, "cut %lld: %lld samples out of range", (long long)b, (long long)L);
    if (idx >= bank->num) return fail(HIPFEAT_ERR_INVALID, "cut %lld: bank index %d of %d", (long long)b, idx, bank->num);
    int64_t o = h_offsets[b], n = L;
    if (h_offsets[b] < 0 || h_offsets[b] + L > tail_start)  // (also the unperturbed cuts: the tail is about to be written)
      return fail(HIPFEAT_ERR_INVALID, "cut %lld (offset %lld, %lld samples) reaches into the arena's tail (tail_start %lld)", (long long)b, (long long)h_offsets[b],
                  (long long)L, (long long)tail_start);
    if (idx >= 0) {
      const int64_t ol = hipfeat_resampled_length(L, bank->orig[idx], bank->nw[idx]);
      s.res.push_back(ResCut{h_offsets[b], tail, (int32_t)L, (int32_t)ol, (int32_t)blocks, bank->kind[idx]});
      blocks += (ol + bank->outs[idx] - 1) / bank->outs[idx];
      if (blocks > INT32_MAX - (1 << 24)) return fail(HIPFEAT_ERR_INVALID, "batch too large for one launch");
      o = tail;
      n = ol;
      tail += (ol + 3) & ~(int64_t)3;
    }
    if (h_max_samples && h_max_samples[b] >= 0) n = std::min(n, h_max_samples[b]);  // a sample or two to truncate (lhotse/audio/recording.py:1058-1060)
    offs[(size_t)b] = o;
    lens[(size_t)b] = n;
    max_len = std::max(max_len, n);
  }
  if (zero_pad_batch) {  // edge_rule "batch_zero_pad" (_extract_batch, extractors.py:531-537): the longest cut of the cut's own mini-batch
    padded.resize((size_t)batch);
    for (size_t k = 0; k + 1 < s.group_first.size(); ++k) {
      int64_t m = 0;
      for (int64_t b = s.group_first[k]; b < s.group_first[k + 1]; ++b) m = std::max(m, lens[(size_t)b]);
      for (int64_t b = s.group_first[k]; b < s.group_first[k + 1]; ++b) padded[(size_t)b] = m;
    }
  }
  (void)max_len;
  hipfeat_status st = build_descs(plan, batch, offs.data(), lens.data(), zero_pad_batch ? padded.data() : nullptr, nullptr, plan->feature_dim, s.descs, &s.lay);
  if (st != HIPFEAT_OK) return st;
  s.lay.owns = false;
  s.res_blocks = blocks;
  s.arena_need = s.res.empty() ? tail_start : tail;  // (nothing to resample: the tail is not touched, its 16-byte alignment slack not needed)
  s.max_frames = 0;
  s.total_rows = 0;
  s.rows.resize((size_t)batch);
  for (size_t k = 0; k + 1 < s.group_first.size(); ++k) {  // every mini-batch = its own dense (B_k, T_k, F) tensor, back to back in d_out
    int64_t tk = 0;
    for (int64_t b = s.group_first[k]; b < s.group_first[k + 1]; ++b) tk = std::max(tk, s.lay.num_frames[(size_t)b]);
    for (int64_t b = s.group_first[k]; b < s.group_first[k + 1]; ++b) {
      s.rows[(size_t)b] = (int32_t)tk;
      s.descs[(size_t)b].out_row = s.total_rows + (b - s.group_first[k]) * tk;
    }
    if (h_group_rows) {
      h_group_rows[2 * k] = s.total_rows;
      h_group_rows[2 * k + 1] = tk;
    }
    s.total_rows += (s.group_first[k + 1] - s.group_first[k]) * tk;
    s.max_frames = std::max(s.max_frames, tk);
  }
  for (int64_t b = 0; b < batch; ++b) {
    if (h_out_offsets) h_out_offsets[b] = offs[(size_t)b];
    if (h_out_num_samples) h_out_num_samples[b] = lens[(size_t)b];
    if (h_num_frames) h_num_frames[b] = s.lay.num_frames[(size_t)b];
  }
  s.planned = true;
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.max_frames;
  h_info[3] = s.total_rows;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_minibatch_run(hipfeat_speed_bank* bank, int64_t ticket, float* d_arena, int64_t arena_floats,
                                                            float* d_out, int64_t rows_per_cut, float pad_value, void* stream) {
  if (!bank || !d_arena || !d_out) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  static const int dbg_skip = exp_env("HIPFEAT_MB_SKIP") ? atoi(exp_env("HIPFEAT_MB_SKIP")) : 0;  // experiments: 1 = no feature launch, 2 = no prep launch
  std::lock_guard<std::mutex> lk(bank->mu);
  MbSlot& s = bank->slots[((ticket % kMbSlots) + kMbSlots) % kMbSlots];
  if (s.ticket != ticket || !s.planned)
    return fail(HIPFEAT_ERR_INVALID, "ticket %lld is not a planned mini-batch (at most %d plans may be outstanding)", (long long)ticket, kMbSlots);
  s.planned = false;
  const hipfeat_plan* plan = s.plan;
  const int64_t batch = s.lay.batch;
  if (arena_floats < s.arena_need) return fail(HIPFEAT_ERR_INVALID, "arena holds %lld floats, the perturbed mini-batch needs %lld", (long long)arena_floats, (long long)s.arena_need);
  const bool grouped = s.group_first.size() > 2;
  if (grouped ? rows_per_cut >= 0 : rows_per_cut < s.max_frames)
    return fail(HIPFEAT_ERR_INVALID, grouped ? "a grouped plan fixes the rows per cut of every mini-batch (h_group_rows): pass rows_per_cut = -1 (got %lld; longest cut %lld frames)"
                                             : "the collated output holds %lld rows per cut, the longest cut has %lld frames", (long long)rows_per_cut, (long long)s.max_frames);
  if (!grouped)
    for (int64_t b = 0; b < batch; ++b) {
      s.descs[(size_t)b].out_row = b * rows_per_cut;
      s.rows[(size_t)b] = (int32_t)rows_per_cut;
    }
  DeviceGuard g(plan->device);
  hipStream_t st = (hipStream_t)stream;
  // padding items: 16 KB pieces of every cut's padding rows
  const int F = plan->feature_dim;
  s.fill_first.resize((size_t)batch + 1);
  int64_t fill_items = 0;
  for (int64_t b = 0; b < batch; ++b) {
    s.fill_first[(size_t)b] = (int32_t)fill_items;
    fill_items += ((int64_t)(s.rows[(size_t)b] - s.descs[(size_t)b].num_frames) * F + kMbFillFloats - 1) / kMbFillFloats;
    if (fill_items > INT32_MAX - (1 << 24)) return fail(HIPFEAT_ERR_INVALID, "batch too large for one launch");
  }
  s.fill_first[(size_t)batch] = (int32_t)fill_items;
  const size_t res_bytes = s.res.size() * sizeof(ResCut), cut_bytes = (size_t)batch * sizeof(CutDesc), fill_bytes = ((size_t)batch + 1) * sizeof(int32_t),
               row_bytes = (size_t)batch * sizeof(int32_t), bytes = (res_bytes + cut_bytes + fill_bytes + row_bytes + 15) & ~(size_t)15;
  const TableRoute route = table_route(bank->allow_inline, bytes);
  const bool inl = route.inl;
  const size_t map_bytes = ((size_t)s.lay.total_blocks * sizeof(int32_t) + 15) & ~(size_t)15;  // the feature launch's workgroup -> cut map
  const size_t dev_bytes = cut_bytes + map_bytes + bytes;  // the feature launch's CutDesc table and map, then (staged path) the blob
  HIP_TRY(s.wait());  // the launches that used this slot's device table last time
  HIP_TRY(s.reserve(dev_bytes));
  s.lay.d_cuts = static_cast<CutDesc*>(s.d);
  // a few workgroups per CU take the items round-robin; the grid is the smallest one that gives every workgroup the same number of items
  static const int64_t mb_slots = exp_env("HIPFEAT_MB_SLOTS") ? std::max(1, atoi(exp_env("HIPFEAT_MB_SLOTS"))) : 1792;
  const int64_t items = fill_items + s.res_blocks;
  const unsigned grid = items_grid(items, mb_slots);
  MbInlineArgs args;  // (header + 3.3 KB; only the used part of the blob is written)
  MbHeader& h = args.h;
  h.arena = d_arena;
  h.out = d_out;
  h.cuts_dst = static_cast<CutDesc*>(s.d);
  h.tables = nullptr;
  for (int k = 0; k < kMbKinds; ++k) h.kt[k] = bank->kt[k];
  h.num_cuts = (int32_t)batch;
  h.num_res = (int32_t)s.res.size();
  h.fill_items = (int32_t)fill_items;
  h.res_items = (int32_t)s.res_blocks;
  h.table_bytes = (int32_t)bytes;
  h.copy_descs = inl ? 1 : 0;
  h.feature_dim = F;
  h.pad_value = pad_value;
  h.feature_blocks = (int32_t)s.lay.total_blocks;
  h.quads_per_wg = s.lay.flat ? (int32_t)(s.lay.fpb / 4) : 0;
  s.lay.uniform_bpc = -1;  // (the map is always there, uniform or not)
  auto fill_blob = [&](unsigned char* dst) {
    if (res_bytes) std::memcpy(dst, s.res.data(), res_bytes);
    std::memcpy(dst + res_bytes, s.descs.data(), cut_bytes);
    std::memcpy(dst + res_bytes + cut_bytes, s.fill_first.data(), fill_bytes);
    std::memcpy(dst + res_bytes + cut_bytes + fill_bytes, s.rows.data(), row_bytes);
  };
  hipError_t e1 = hipSuccess;
  auto fill_map = [&](unsigned char* dst) {
    int32_t* m = reinterpret_cast<int32_t*>(dst);
    if (s.lay.flat) {  // (laid out by frame quads: the map build_descs computed)
      std::memcpy(m, s.lay.block_cut.data(), s.lay.block_cut.size() * sizeof(int32_t));
      return;
    }
    for (int64_t b = 0; b < batch; ++b) {
      const int64_t b0 = s.descs[(size_t)b].first_block, b1 = b + 1 < batch ? s.descs[(size_t)b + 1].first_block : s.lay.total_blocks;
      std::fill(m + b0, m + b1, (int32_t)b);
    }
  };
  if (dbg_skip == 2) {  // (experiments: no prep launch; the descriptor table of the feature launch still has to get there)
    std::memcpy(s.h, s.descs.data(), cut_bytes);
    fill_map(static_cast<unsigned char*>(s.h) + cut_bytes);
    HIP_TRY(hipMemcpyAsync(s.d, s.h, cut_bytes + map_bytes, hipMemcpyHostToDevice, st));
  } else if (inl) {
    fill_blob(args.blob);
    hipLaunchKernelGGL(minibatch_prep_inline_kernel, dim3(grid), dim3(256), 0, st, args);
    e1 = hipGetLastError();
  } else {
    unsigned char* hb = static_cast<unsigned char*>(s.h);
    std::memcpy(hb, s.descs.data(), cut_bytes);
    fill_map(hb + cut_bytes);
    fill_blob(hb + cut_bytes + map_bytes);
    HIP_TRY(hipMemcpyAsync(s.d, s.h, dev_bytes, hipMemcpyHostToDevice, st));
    h.tables = static_cast<const unsigned char*>(s.d) + cut_bytes + map_bytes;
    hipLaunchKernelGGL(minibatch_prep_kernel, dim3(grid), dim3(256), route.dyn, st, h);
    e1 = hipGetLastError();
  }
  hipfeat_status rc = HIPFEAT_OK;
  if (e1 != hipSuccess) rc = fail(HIPFEAT_ERR_HIP, "mini-batch prep launch failed: %s", hipGetErrorName(e1));
  if (rc == HIPFEAT_OK && s.lay.total_blocks > 0 && dbg_skip != 1) rc = launch(plan, &s.lay, d_arena, d_out, st);
  (void)s.record(st);
  return rc;
}

// --------------------------------------------------------------------------------------
// MixedCut tracks mixed on the device: energies, gains and the scaled sum in two launches (kernel_mix.hpp; the tables: mix_tables.hpp)
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_API hipfeat_status hipfeat_mixer_create(int32_t device, hipfeat_mixer** out) { return handle_create(device, out, "mixer"); }
extern "C" HIPFEAT_API hipfeat_status hipfeat_mixer_destroy(hipfeat_mixer* m) { return handle_destroy(m); }

extern "C" HIPFEAT_API hipfeat_status hipfeat_mix_plan(hipfeat_mixer* mixer, int64_t num_cuts, const int64_t* h_track_first, const int64_t* h_src_offset,
                                                       const int64_t* h_src_len, const int64_t* h_dst_offset, const double* h_snr_db,
                                                       const int32_t* h_ref_track, const int64_t* h_max_samples, int64_t tail_start,
                                                       int64_t* h_out_offsets, int64_t* h_out_num_samples, int64_t* h_info) {
  if (!mixer || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  // (validated into a local first: a refused table leaves the outstanding plans as they were)
  MixPlan p = build_mix_plan(num_cuts, h_track_first, h_src_offset, h_src_len, h_dst_offset, h_snr_db, h_ref_track, h_max_samples, tail_start);
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  std::lock_guard<std::mutex> lk(mixer->mu);
  int64_t ticket;
  if (hipfeat_status st = take_ticket(mixer->tickets, "mixes", &ticket)) return st;
  const MixPlan& s = mixer->plans[ticket % kTicketSlots] = std::move(p);
  for (int64_t c = 0; c < num_cuts; ++c) {
    if (h_out_offsets) h_out_offsets[c] = s.cuts[(size_t)c].out_off;
    if (h_out_num_samples) h_out_num_samples[c] = s.cuts[(size_t)c].out_len;
  }
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.energy_items;
  h_info[3] = s.mix_items;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_mix_run(hipfeat_mixer* mixer, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream) {
  if (!mixer || !d_arena) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(mixer->mu);
  const int slot = find_ticket(mixer->tickets, ticket, "mix");
  if (slot < 0) return HIPFEAT_ERR_INVALID;
  const MixPlan& p = mixer->plans[slot];
  StagedSlot& s = mixer->slots[slot];  // device: the staged tables, then the partial sums of squares
  if (arena_floats < p.arena_need)
    return fail(HIPFEAT_ERR_INVALID, "arena holds %lld floats, the mixed cuts need %lld", (long long)arena_floats, (long long)p.arena_need);
  if (reinterpret_cast<uintptr_t>(d_arena) & 15) return fail(HIPFEAT_ERR_INVALID, "the arena must start on a 16-byte boundary");
  DeviceGuard g(mixer->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t cut_bytes = p.cuts.size() * sizeof(MixCut), trk_bytes = p.tracks.size() * sizeof(MixTrack), bytes = cut_bytes + trk_bytes;  // (multiples of 32)
  const size_t part_bytes = (size_t)std::max<int64_t>(p.energy_items, 1) * sizeof(double);
  const TableRoute r = table_route(mixer->allow_inline, bytes);
  HIP_TRY(s.wait());
  HIP_TRY(s.reserve(bytes + part_bytes));
  MixInlineArgs args;  // (header + 3.3 KB; only the used part of the blob is written)
  MixHeader& h = args.h;
  h.arena = d_arena;
  h.partials = reinterpret_cast<double*>(static_cast<unsigned char*>(s.d) + bytes);
  h.num_cuts = (int32_t)p.cuts.size();
  h.num_tracks = (int32_t)p.tracks.size();
  h.energy_items = (int32_t)p.energy_items;
  h.mix_items = (int32_t)p.mix_items;
  h.table_bytes = (int32_t)bytes;
  h.pad = 0;
  HIP_TRY(place_tables(args, r, s, bytes, st, [&](unsigned char* dst) {
    std::memcpy(dst, p.cuts.data(), cut_bytes);
    std::memcpy(dst + cut_bytes, p.tracks.data(), trk_bytes);
  }));
  const dim3 energy_grid(items_grid(p.energy_items)), mix_grid(items_grid(p.mix_items)), wg(256);
  if (r.inl) {
    if (p.energy_items > 0) hipLaunchKernelGGL(mix_energy_inline_kernel, energy_grid, wg, 0, st, args);
    hipLaunchKernelGGL(mix_inline_kernel, mix_grid, wg, 0, st, args);
  } else {
    if (p.energy_items > 0) hipLaunchKernelGGL(mix_energy_kernel, energy_grid, wg, r.dyn, st, h);
    hipLaunchKernelGGL(mix_kernel, mix_grid, wg, r.dyn, st, h);
  }
  mixer->tickets.release(ticket);
  return finish_launches(s, st, hipGetLastError(), "mix", kWaitedLaunches);
}

// --------------------------------------------------------------------------------------
// Reverberation with a recorded impulse response on the device: convolution + power normalisation in two launches (kernel_reverb.hpp;
// the table: reverb_tables.hpp)
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_API hipfeat_status hipfeat_reverb_create(int32_t device, hipfeat_reverb** out) { return handle_create(device, out, "reverb"); }
extern "C" HIPFEAT_API hipfeat_status hipfeat_reverb_destroy(hipfeat_reverb* r) {
  if (r && (r->d_tw || r->d_tw64)) {
    DeviceGuard g(r->device);
    for (auto& s : r->slots) (void)s.wait();  // the launches that read the twiddles are done
    if (r->d_tw) (void)hipFree(r->d_tw);
    if (r->d_tw64) (void)hipFree(r->d_tw64);
  }
  return handle_destroy(r);
}

// a validated plan of either entry point into the handle's ring: the ticket, the output offsets and the info fields
static hipfeat_status reverb_keep_plan(hipfeat_reverb* rv, RvMethodPlan&& p, int64_t num_items, int64_t* h_out_offsets, int64_t* h_info, bool method_info) {
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  std::lock_guard<std::mutex> lk(rv->mu);
  int64_t ticket;
  if (hipfeat_status st = take_ticket(rv->tickets, "reverberations", &ticket)) return st;
  const RvMethodPlan& s = rv->plans[ticket % kTicketSlots] = std::move(p);
  if (h_out_offsets)
    for (int64_t i = 0; i < num_items; ++i) h_out_offsets[i] = s.out_offsets[(size_t)i];
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.work_items;
  h_info[3] = 2 * s.work_items + s.fft_partials();
  if (method_info) {
    h_info[4] = s.fft.a_work;
    h_info[5] = s.fft.b_work;
    h_info[6] = s.fft.g_work;
    h_info[7] = (int64_t)s.fft.rirs.size();
  }
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_reverb_plan(hipfeat_reverb* rv, int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len,
                                                          const int64_t* h_rir_offset, const int64_t* h_rir_len, const int64_t* h_shift,
                                                          const int32_t* h_normalize, int64_t tail_start, int64_t* h_out_offsets, int64_t* h_info) {
  if (!rv || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  // (validated into a local first: a refused table leaves the outstanding plans as they were)
  return reverb_keep_plan(rv, build_reverb_plan_method(num_items, h_src_offset, h_src_len, h_rir_offset, h_rir_len, h_shift, h_normalize, tail_start, kRvDirect, 0),
                          num_items, h_out_offsets, h_info, false);
}

extern "C" HIPFEAT_REVERB_FFT_API hipfeat_status hipfeat_reverb_plan_method(hipfeat_reverb* rv, int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len,
                                                                 const int64_t* h_rir_offset, const int64_t* h_rir_len, const int64_t* h_shift,
                                                                 const int32_t* h_normalize, int64_t tail_start, int32_t method, int64_t min_fft_taps,
                                                                 int64_t* h_out_offsets, int64_t* h_info) {
  if (!rv || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  return reverb_keep_plan(rv, build_reverb_plan_method(num_items, h_src_offset, h_src_len, h_rir_offset, h_rir_len, h_shift, h_normalize, tail_start, method,
                                                       min_fft_taps),
                          num_items, h_out_offsets, h_info, true);
}

// the FFT items of a ticket: spectra, accumulate and invert, gain (kernel_reverb_fft.hpp); their table and partial sums lie in the
// ticket's slot from byte `foff` on (reserved by the caller)
static size_t rf_table_bytes(const RfPlan& f) { return f.items.size() * sizeof(RfItem) + f.rirs.size() * sizeof(RfRir); }

static hipfeat_status reverb_run_fft(hipfeat_reverb* rv, const RfPlan& f, StagedSlot& s, size_t foff, float* d_arena, hipStream_t st) {
  const size_t fbytes = rf_table_bytes(f);
  const TableRoute fr = table_route(rv->allow_inline, fbytes);
  if (!rv->d_tw) {  // once per handle
    const std::vector<float2> tw = fft_twiddles(2 * kRfBlock, kRfBlock);
    std::vector<double2> tw64((size_t)kRfBlock);  // W_2048^k in float64: the RIR spectra and the inverse transform run in it
    for (int k = 0; k < kRfBlock; ++k) {
      const double a = -2.0 * M_PI * (double)k / (double)(2 * kRfBlock);
      tw64[(size_t)k] = make_double2(std::cos(a), std::sin(a));
    }
    if (!rv->d_tw64)
      if (hipfeat_status bad = upload(&rv->d_tw64, tw64.data(), tw64.size())) return bad;
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(rf_spectra_kernel), kRfMaxTableLds));
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(rf_rir_inline_kernel), kRfLds64));
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(rf_output_inline_kernel), kRfLds64));
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(rf_rir_kernel), kRfLds64 + kRfMaxTableLds));
    HIP_TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(rf_output_kernel), kRfLds64 + kRfMaxTableLds));
    if (hipfeat_status bad = upload(&rv->d_tw, tw.data(), tw.size())) return bad;  // (last: d_tw says that all of this is done)
  }
  RfInlineArgs fa;  // (only the used part of the blob is written)
  RfHeader& fh = fa.h;
  fh.arena = d_arena;
  fh.partials = reinterpret_cast<double*>(static_cast<unsigned char*>(s.d) + foff + fbytes);
  fh.tw = rv->d_tw;
  fh.tw64 = rv->d_tw64;
  fh.num_items = (int32_t)f.items.size();
  fh.num_rirs = (int32_t)f.rirs.size();
  fh.table_bytes = (int32_t)fbytes;
  fh.rir_work = (int32_t)f.rir_work;
  fh.a_work = (int32_t)f.a_work;
  fh.b_work = (int32_t)f.b_work;
  fh.g_work = (int32_t)f.g_work;
  fh.x_total = (int32_t)f.x_total;
  fh.tables = fr.inl ? nullptr : static_cast<const unsigned char*>(s.d) + foff;
  unsigned char* dst = fr.inl ? fa.blob : static_cast<unsigned char*>(s.h) + foff;
  std::memcpy(dst, f.items.data(), f.items.size() * sizeof(RfItem));
  std::memcpy(dst + f.items.size() * sizeof(RfItem), f.rirs.data(), f.rirs.size() * sizeof(RfRir));
  if (!fr.inl) HIP_TRY(hipMemcpyAsync(static_cast<unsigned char*>(s.d) + foff, dst, fbytes, hipMemcpyHostToDevice, st));
  const dim3 wg(256), gr(items_grid((f.rir_work + kRfWaves - 1) / kRfWaves, kRfGridSlots)), ga(items_grid((f.x_total + kRfWaves - 1) / kRfWaves, kRfGridSlots)),
      gb(items_grid((f.b_work + kRfWaves - 1) / kRfWaves, kRfGridSlots)), gg(items_grid(f.g_work));
  if (fr.inl) {
    hipLaunchKernelGGL(rf_rir_inline_kernel, gr, wg, kRfLds64, st, fa);
    hipLaunchKernelGGL(rf_spectra_inline_kernel, ga, wg, 0, st, fa);
    hipLaunchKernelGGL(rf_output_inline_kernel, gb, wg, kRfLds64, st, fa);
    hipLaunchKernelGGL(rf_gain_inline_kernel, gg, wg, 0, st, fa);
  } else {
    hipLaunchKernelGGL(rf_rir_kernel, gr, wg, kRfLds64 + fr.dyn, st, fh);
    hipLaunchKernelGGL(rf_spectra_kernel, ga, wg, fr.dyn, st, fh);
    hipLaunchKernelGGL(rf_output_kernel, gb, wg, kRfLds64 + fr.dyn, st, fh);
    hipLaunchKernelGGL(rf_gain_kernel, gg, wg, fr.dyn, st, fh);
  }
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_reverb_run(hipfeat_reverb* rv, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream) {
  if (!rv || !d_arena) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(rv->mu);
  const int slot = find_ticket(rv->tickets, ticket, "reverberation");
  if (slot < 0) return HIPFEAT_ERR_INVALID;
  const RvMethodPlan& p = rv->plans[slot];
  StagedSlot& s = rv->slots[slot];  // device: the staged table, then the partial sums of squares; behind them the same of the FFT items
  if (arena_floats < p.arena_need)
    return fail(HIPFEAT_ERR_INVALID, "arena holds %lld floats, the reverberated cuts need %lld", (long long)arena_floats, (long long)p.arena_need);
  if (reinterpret_cast<uintptr_t>(d_arena) & 15) return fail(HIPFEAT_ERR_INVALID, "the arena must start on a 16-byte boundary");
  DeviceGuard g(rv->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = p.items.size() * sizeof(RvItem);  // (a multiple of 16)
  const size_t part_bytes = (size_t)p.work_items * 2 * sizeof(double);
  const TableRoute r = table_route(rv->allow_inline, bytes);
  const RfPlan& f = p.fft;
  const size_t fbytes = rf_table_bytes(f), foff = bytes + part_bytes;  // (multiples of 16)
  HIP_TRY(s.wait());
  HIP_TRY(s.reserve(foff + fbytes + (size_t)p.fft_partials() * sizeof(double)));
  RvInlineArgs args;  // (header + 3.3 KB; only the used part of the blob is written)
  RvHeader& h = args.h;
  h.arena = d_arena;
  h.partials = reinterpret_cast<double*>(static_cast<unsigned char*>(s.d) + bytes);
  h.num_items = (int32_t)p.items.size();
  h.work_items = (int32_t)p.work_items;
  h.table_bytes = (int32_t)bytes;
  h.pad = 0;
  HIP_TRY(place_tables(args, r, s, bytes, st, [&](unsigned char* dst) { std::memcpy(dst, p.items.data(), bytes); }));
  const dim3 grid(items_grid(p.work_items)), wg(256);
  if (p.items.empty()) {
    // (every item of the ticket takes the FFT route)
  } else if (r.inl) {
    hipLaunchKernelGGL(reverb_conv_inline_kernel, grid, wg, 0, st, args);
    hipLaunchKernelGGL(reverb_gain_inline_kernel, grid, wg, 0, st, args);
  } else {
    hipLaunchKernelGGL(reverb_conv_kernel, grid, wg, r.dyn, st, h);
    hipLaunchKernelGGL(reverb_gain_kernel, grid, wg, r.dyn, st, h);
  }
  if (!f.items.empty())
    if (hipfeat_status bad = reverb_run_fft(rv, f, s, foff, d_arena, st)) return bad;
  rv->tickets.release(ticket);
  return finish_launches(s, st, hipGetLastError(), "reverb", kWaitedLaunches);
}

// --------------------------------------------------------------------------------------
// Level changes on the device (Volume, Clipping): peak + apply in two launches (kernel_level.hpp; the table: level_tables.hpp)
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_API hipfeat_status hipfeat_level_create(int32_t device, hipfeat_level** out) { return handle_create(device, out, "level"); }
extern "C" HIPFEAT_API hipfeat_status hipfeat_level_destroy(hipfeat_level* l) { return handle_destroy(l); }

extern "C" HIPFEAT_API hipfeat_status hipfeat_level_plan(hipfeat_level* lv, int64_t num_items, const int64_t* h_src_offset, const int64_t* h_src_len,
                                                         const int64_t* h_dst_offset, const int64_t* h_op_first, const int32_t* h_op_kind,
                                                         const float* h_op_value, const int32_t* h_op_flags, int64_t* h_info) {
  if (!lv || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  // (validated into a local first: a refused table leaves the outstanding plans as they were)
  LvPlan p = build_level_plan(num_items, h_src_offset, h_src_len, h_dst_offset, h_op_first, h_op_kind, h_op_value, h_op_flags);
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  std::lock_guard<std::mutex> lk(lv->mu);
  int64_t ticket;
  if (hipfeat_status st = take_ticket(lv->tickets, "level changes", &ticket)) return st;
  const LvPlan& s = lv->plans[ticket % kTicketSlots] = std::move(p);
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.peak_items;
  h_info[3] = s.work_items;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_level_run(hipfeat_level* lv, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream) {
  if (!lv) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(lv->mu);
  const int slot = find_ticket(lv->tickets, ticket, "level change");
  if (slot < 0) return HIPFEAT_ERR_INVALID;
  const LvPlan& p = lv->plans[slot];
  StagedSlot& s = lv->slots[slot];  // device: the staged table, then the partial peaks
  if (p.items.empty()) {  // nothing to do: no launch
    lv->tickets.release(ticket);
    return HIPFEAT_OK;
  }
  if (!d_arena) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (arena_floats < p.arena_need)
    return fail(HIPFEAT_ERR_INVALID, "arena holds %lld floats, the items reach to %lld", (long long)arena_floats, (long long)p.arena_need);
  if (reinterpret_cast<uintptr_t>(d_arena) & 15) return fail(HIPFEAT_ERR_INVALID, "the arena must start on a 16-byte boundary");
  DeviceGuard g(lv->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = p.items.size() * sizeof(LvItem);  // (a multiple of 16)
  const size_t part_bytes = (size_t)p.work_items * sizeof(float);
  const TableRoute r = table_route(lv->allow_inline, bytes);
  HIP_TRY(s.wait());
  HIP_TRY(s.reserve(bytes + part_bytes));
  LvInlineArgs args;  // (header + 3.3 KB; only the used part of the blob is written)
  LvHeader& h = args.h;
  h.arena = d_arena;
  h.partials = reinterpret_cast<float*>(static_cast<unsigned char*>(s.d) + bytes);
  h.num_items = (int32_t)p.items.size();
  h.work_items = (int32_t)p.work_items;
  h.table_bytes = (int32_t)bytes;
  h.pad = 0;
  HIP_TRY(place_tables(args, r, s, bytes, st, [&](unsigned char* dst) { std::memcpy(dst, p.items.data(), bytes); }));
  const dim3 grid(items_grid(p.work_items)), wg(256);
  bool any_clip = false;
  for (const LvItem& it : p.items) any_clip = any_clip || it.clip_at >= 0;
  if (r.inl) {
    if (any_clip) hipLaunchKernelGGL(level_peak_inline_kernel, grid, wg, 0, st, args);
    hipLaunchKernelGGL(level_apply_inline_kernel, grid, wg, 0, st, args);
  } else {
    if (any_clip) hipLaunchKernelGGL(level_peak_kernel, grid, wg, r.dyn, st, h);
    hipLaunchKernelGGL(level_apply_kernel, grid, wg, r.dyn, st, h);
  }
  lv->tickets.release(ticket);
  return finish_launches(s, st, hipGetLastError(), "level", kWaitedLaunches);
}

// --------------------------------------------------------------------------------------
// Collation on the device (AudioSamples, return_audio): one launch (kernel_collate.hpp; the table: collate_tables.hpp)
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_create(int32_t device, hipfeat_collate** out) { return handle_create(device, out, "collate"); }
extern "C" HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_destroy(hipfeat_collate* c) { return handle_destroy(c); }

extern "C" HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_plan(hipfeat_collate* c, int64_t num_rows, const int64_t* h_src_offset, const int64_t* h_src_len,
                                                                   const int64_t* h_dst_offset, int64_t row_len, int32_t out_type, int64_t* h_info) {
  if (!c || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  // (validated into a local first: a refused table leaves the outstanding plans as they were)
  CoPlan p = build_collate_plan(num_rows, h_src_offset, h_src_len, h_dst_offset, row_len, out_type);
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  std::lock_guard<std::mutex> lk(c->mu);
  int64_t ticket;
  if (hipfeat_status st = take_ticket(c->tickets, "collations", &ticket)) return st;
  const CoPlan& s = c->plans[ticket % kTicketSlots] = std::move(p);
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.out_need;
  h_info[3] = s.work_items;
  return HIPFEAT_OK;
}

// the sources form: a row is the mean of k >= 0 runs of the arena (collate_audio's mono_downmix, collation.py:215-241)
extern "C" HIPFEAT_CHANNELS_API hipfeat_status hipfeat_collate_plan_sources(hipfeat_collate* c, int64_t num_rows, const int64_t* h_first,
                                                                            const int64_t* h_src_offset, const int64_t* h_src_len,
                                                                           const int64_t* h_dst_offset, int64_t row_len, int32_t out_type,
                                                                           int64_t* h_info) {
  if (!c || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  CoPlan p = build_collate_sources_plan(num_rows, h_first, h_src_offset, h_src_len, h_dst_offset, row_len, out_type);
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  std::lock_guard<std::mutex> lk(c->mu);
  int64_t ticket;
  if (hipfeat_status st = take_ticket(c->tickets, "collations", &ticket)) return st;
  const CoPlan& s = c->plans[ticket % kTicketSlots] = std::move(p);
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.out_need;
  h_info[3] = s.work_items;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_COLLATE_API hipfeat_status hipfeat_collate_run(hipfeat_collate* c, int64_t ticket, const float* d_arena, int64_t arena_floats, void* d_out,
                                                                  int64_t out_elements, void* stream) {
  if (!c) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(c->mu);
  const int slot = find_ticket(c->tickets, ticket, "collation");
  if (slot < 0) return HIPFEAT_ERR_INVALID;
  const CoPlan& p = c->plans[slot];
  StagedSlot& s = c->slots[slot];  // device: the row table
  if (arena_floats < p.arena_need)
    return fail(HIPFEAT_ERR_INVALID, "arena holds %lld floats, the rows read up to %lld", (long long)arena_floats, (long long)p.arena_need);
  if (out_elements < p.out_need)
    return fail(HIPFEAT_ERR_INVALID, "out holds %lld elements, the rows take %lld", (long long)out_elements, (long long)p.out_need);
  if (p.work_items == 0) {  // no rows, or rows of no elements: no launch
    c->tickets.release(ticket);
    return HIPFEAT_OK;
  }
  const int esz = co_elem_bytes(p.out_type);
  if (!d_out || (!d_arena && p.arena_need > 0)) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(d_arena) & 15) return fail(HIPFEAT_ERR_INVALID, "the arena must start on a 16-byte boundary");
  if (reinterpret_cast<uintptr_t>(d_out) & (uintptr_t)(esz - 1)) return fail(HIPFEAT_ERR_INVALID, "out must be aligned to its element size");
  {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(d_arena), a1 = a0 + (uintptr_t)arena_floats * 4;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + (uintptr_t)out_elements * (uintptr_t)esz;
    if (a0 < o1 && o0 < a1) return fail(HIPFEAT_ERR_INVALID, "out overlaps the arena");
  }
  DeviceGuard g(c->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = p.rows.size() * sizeof(CoRow);
  // a flat 1-D grid over (row, tile); beyond 2^22 workgroups (2^34 elements) the workgroups stride
  const unsigned grid = (unsigned)std::min<int64_t>(p.work_items, (int64_t)1 << 22);
  if (p.sources) {  // the row table, and behind it the source offsets of all rows
    const size_t src_bytes = p.srcs.size() * sizeof(int64_t);
    HIP_TRY(stage(s, bytes + src_bytes, bytes + src_bytes, st, [&](unsigned char* h) {
      std::memcpy(h, p.rows.data(), bytes);
      if (src_bytes) std::memcpy(h + bytes, p.srcs.data(), src_bytes);
    }));
    CoMeanArgs m;
    m.arena = reinterpret_cast<const uint32_t*>(d_arena);
    m.out = d_out;
    m.rows = static_cast<const CoRow*>(s.d);
    m.srcs = reinterpret_cast<const int64_t*>(static_cast<const unsigned char*>(s.d) + bytes);
    m.row_len = p.row_len;
    m.tiles_per_row = p.tiles_per_row;
    m.work_items = p.work_items;
    if (p.out_type == kCoF32) hipLaunchKernelGGL(collate_mean_kernel<float>, dim3(grid), dim3(256), 0, st, m);
    else if (p.out_type == kCoF16) hipLaunchKernelGGL(collate_mean_kernel<__half>, dim3(grid), dim3(256), 0, st, m);
    else hipLaunchKernelGGL(collate_mean_kernel<__hip_bfloat16>, dim3(grid), dim3(256), 0, st, m);
    c->tickets.release(ticket);
    return finish_launches(s, st, hipGetLastError(), "collate", kWaitedLaunch);
  }
  HIP_TRY(stage(s, bytes, bytes, st, [&](unsigned char* h) { std::memcpy(h, p.rows.data(), bytes); }));
  CoArgs a;
  a.arena = reinterpret_cast<const uint32_t*>(d_arena);
  a.out = d_out;
  a.rows = static_cast<const CoRow*>(s.d);
  a.row_len = p.row_len;
  a.tiles_per_row = p.tiles_per_row;
  a.work_items = p.work_items;
  if (p.out_type == kCoF32) hipLaunchKernelGGL(collate_wave_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  else if (p.out_type == kCoF16) hipLaunchKernelGGL(collate_wave_kernel<__half>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(collate_wave_kernel<__hip_bfloat16>, dim3(grid), dim3(256), 0, st, a);
  c->tickets.release(ticket);
  return finish_launches(s, st, hipGetLastError(), "collate", kWaitedLaunch);
}

// --------------------------------------------------------------------------------------
// Sinc resampler without a filter bank (LowpassUsingResampling, any Resample): one launch (kernel_sinc.hpp; the table: sinc_tables.hpp)
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_create(int32_t device, hipfeat_sinc** out) { return handle_create(device, out, "sinc"); }
extern "C" HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_destroy(hipfeat_sinc* sc) { return handle_destroy(sc); }

extern "C" HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_plan(hipfeat_sinc* sc, int64_t num_rows, const int64_t* h_in_offset, const int64_t* h_in_len,
                                                             const int32_t* h_src_rate, const int32_t* h_dst_rate, const int64_t* h_out_offset,
                                                             int64_t arena_floats, int64_t* h_out_len, int64_t* h_info) {
  if (!sc || !h_info || (num_rows > 0 && !h_out_len)) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  // (validated into a local first: a refused table leaves the outstanding plans as they were)
  SincPlan p = build_sinc_plan(num_rows, h_in_offset, h_in_len, h_src_rate, h_dst_rate, h_out_offset, arena_floats);
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  std::lock_guard<std::mutex> lk(sc->mu);
  int64_t ticket;
  if (hipfeat_status st = take_ticket(sc->tickets, "resamplings", &ticket)) return st;
  const SincPlan& s = sc->plans[ticket % kTicketSlots] = std::move(p);
  for (int64_t i = 0; i < num_rows; ++i) h_out_len[i] = s.out_len[(size_t)i];
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.workgroups;
  h_info[3] = s.max_w;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_run(hipfeat_sinc* sc, int64_t ticket, float* d_arena, int64_t arena_floats, void* stream) {
  if (!sc) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(sc->mu);
  const int slot = find_ticket(sc->tickets, ticket, "resampling");
  if (slot < 0) return HIPFEAT_ERR_INVALID;
  const SincPlan& p = sc->plans[slot];
  StagedSlot& s = sc->slots[slot];  // device: the row table
  if (arena_floats < p.arena_need)
    return fail(HIPFEAT_ERR_INVALID, "arena holds %lld floats, the rows reach to %lld", (long long)arena_floats, (long long)p.arena_need);
  if (p.workgroups == 0) {  // no rows, or rows of no samples: no launch
    sc->tickets.release(ticket);
    return HIPFEAT_OK;
  }
  if (!d_arena) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(d_arena) & 15) return fail(HIPFEAT_ERR_INVALID, "the arena must start on a 16-byte boundary");
  DeviceGuard g(sc->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t bytes = p.rows.size() * sizeof(SincRow);
  const size_t lds = (size_t)p.max_w * kSincPhases * sizeof(float);
  {
    hipError_t e = ensure_dynamic_lds(entry<sinc_kernel>(), lds);
    if (e != hipSuccess) return fail(HIPFEAT_ERR_HIP, "hipFuncSetAttribute(dynamic LDS = %zu B) failed: %s", lds, hipGetErrorName(e));
  }
  HIP_TRY(stage(s, bytes, bytes, st, [&](unsigned char* h) { std::memcpy(h, p.rows.data(), bytes); }));
  SincArgs a;
  a.arena = d_arena;
  a.rows = static_cast<const SincRow*>(s.d);
  a.num_rows = (int32_t)p.rows.size();
  a.pad = 0;
  hipLaunchKernelGGL(sinc_kernel, dim3((unsigned)p.workgroups), dim3(256), lds, st, a);
  sc->tickets.release(ticket);
  return finish_launches(s, st, hipGetLastError(), "sinc", kWaitedLaunch);
}

extern "C" HIPFEAT_SINC_API hipfeat_status hipfeat_sinc_weights(hipfeat_sinc* sc, int32_t src_rate, int32_t dst_rate, float* d_weights, int32_t* d_first,
                                                                int32_t* h_dims, void* stream) {
  if (!sc || !h_dims) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  int32_t dims[4] = {0, 0, 0, 0};
  const int st = sinc_supported(src_rate, dst_rate, dims);
  if (st == 1) return fail(HIPFEAT_ERR_INVALID, "rates %d -> %d: both must be positive and they must differ", src_rate, dst_rate);
  if (st != 0 && dims[3] == 0) return fail(HIPFEAT_ERR_UNSUPPORTED, "%d -> %d: the rates reduced by their gcd must not exceed 2^24", src_rate, dst_rate);
  if (st != 0) return fail(HIPFEAT_ERR_UNSUPPORTED, "%d -> %d needs a window of %d taps per phase, the kernel holds %d", src_rate, dst_rate, dims[3], kSincMaxW);
  h_dims[0] = dims[1];
  h_dims[1] = dims[3];
  h_dims[2] = dims[2];
  if (!d_weights && !d_first) return HIPFEAT_OK;  // the sizes alone
  if (!d_weights || !d_first) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(sc->mu);
  DeviceGuard g(sc->device);
  hipLaunchKernelGGL(sinc_weights_kernel, dim3((unsigned)((dims[1] + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_weights, d_first, dims[0], dims[1], dims[2],
                     sinc_base(dims[0], dims[1]));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(HIPFEAT_ERR_HIP, "sinc weights launch failed: %s", hipGetErrorName(e));
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// Stored features mixed and collated on the device (PrecomputedFeatures + CutMix / .pad): energies, then the fold and the padded
// batch, in two launches (kernel_featmix.hpp; the tables: featmix_tables.hpp)
// --------------------------------------------------------------------------------------
extern "C" HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_create(int32_t device, hipfeat_featmix** out) { return handle_create(device, out, "featmix"); }
extern "C" HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_destroy(hipfeat_featmix* fm) { return handle_destroy(fm); }

extern "C" HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_plan(hipfeat_featmix* fm, int64_t num_cuts, const int64_t* h_track_first, const int32_t* h_form,
                                                                   const int64_t* h_num_frames, const double* h_pad_value, const int64_t* h_dst_first,
                                                                   const int32_t* h_ref_track, const int64_t* h_src_offset, const int64_t* h_src_rows,
                                                                   const int64_t* h_frames, const int32_t* h_dtype, const int64_t* h_first, const double* h_snr_db,
                                                                   const double* h_value, int64_t num_features, int64_t row_frames, int64_t* h_info) {
  if (!fm || !h_info) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  // (validated into a local first: a refused table leaves the outstanding plans as they were)
  FmPlan p = build_featmix_plan(num_cuts, h_track_first, h_form, h_num_frames, h_pad_value, h_dst_first, h_ref_track, h_src_offset, h_src_rows, h_frames, h_dtype,
                                h_first, h_snr_db, h_value, num_features, row_frames);
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  std::lock_guard<std::mutex> lk(fm->mu);
  int64_t ticket;
  if (hipfeat_status st = take_ticket(fm->tickets, "feature mixes", &ticket)) return st;
  const FmPlan& s = fm->plans[ticket % kTicketSlots] = std::move(p);
  h_info[0] = ticket;
  h_info[1] = s.arena_need;
  h_info[2] = s.energy_items;
  h_info[3] = s.fold_items;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_FEATMIX_API hipfeat_status hipfeat_featmix_run(hipfeat_featmix* fm, int64_t ticket, const void* d_arena, int64_t arena_bytes, float* d_out,
                                                                  int64_t out_elements, void* stream) {
  if (!fm) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(fm->mu);
  const int slot = find_ticket(fm->tickets, ticket, "feature mix");
  if (slot < 0) return HIPFEAT_ERR_INVALID;
  const FmPlan& p = fm->plans[slot];
  StagedSlot& s = fm->slots[slot];  // device: the staged tables, then the partial sums
  if (arena_bytes < p.arena_need)
    return fail(HIPFEAT_ERR_INVALID, "arena holds %lld bytes, the tracks reach to %lld", (long long)arena_bytes, (long long)p.arena_need);
  if (out_elements < p.out_need)
    return fail(HIPFEAT_ERR_INVALID, "out holds %lld elements, the batch takes %lld", (long long)out_elements, (long long)p.out_need);
  if (p.fold_items == 0) {  // rows of no frames: no launch
    fm->tickets.release(ticket);
    return HIPFEAT_OK;
  }
  if (!d_out || (!d_arena && p.arena_need > 0)) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(d_arena) & 15) return fail(HIPFEAT_ERR_INVALID, "the arena must start on a 16-byte boundary");
  if (reinterpret_cast<uintptr_t>(d_out) & 3) return fail(HIPFEAT_ERR_INVALID, "out must be aligned to its element size");
  {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(d_arena), a1 = a0 + (uintptr_t)arena_bytes;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + (uintptr_t)out_elements * 4;
    if (a0 < o1 && o0 < a1) return fail(HIPFEAT_ERR_INVALID, "out overlaps the arena");
  }
  DeviceGuard g(fm->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t cut_bytes = p.cuts.size() * sizeof(FmCut), trk_bytes = p.tracks.size() * sizeof(FmTrack), bytes = cut_bytes + trk_bytes;  // (multiples of 16)
  const size_t part_bytes = (size_t)std::max<int64_t>(p.energy_items, 1) * sizeof(double);
  HIP_TRY(stage(s, bytes + part_bytes, bytes, st, [&](unsigned char* h) {
    std::memcpy(h, p.cuts.data(), cut_bytes);
    std::memcpy(h + cut_bytes, p.tracks.data(), trk_bytes);
  }));
  FmArgs a;
  a.arena = static_cast<const unsigned char*>(d_arena);
  a.out = d_out;
  a.cuts = static_cast<const FmCut*>(s.d);
  a.tracks = reinterpret_cast<const FmTrack*>(static_cast<const unsigned char*>(s.d) + cut_bytes);
  a.partials = reinterpret_cast<double*>(static_cast<unsigned char*>(s.d) + bytes);
  a.row_len = p.row_len;
  a.tiles_per_row = p.tiles_per_row;
  a.fold_items = p.fold_items;
  a.num_cuts = (int32_t)p.cuts.size();
  a.num_tracks = (int32_t)p.tracks.size();
  a.energy_items = (int32_t)p.energy_items;
  a.num_features = (int32_t)p.num_features;
  a.log_eps = (float)std::log(1e-10);
  a.pad = 0;
  if (p.energy_items > 0) hipLaunchKernelGGL(featmix_energy_kernel, dim3(items_grid(p.energy_items)), dim3(256), 0, st, a);
  // a flat 1-D grid over (cut, tile); beyond 2^22 workgroups (2^34 elements) the workgroups stride
  hipLaunchKernelGGL(featmix_fold_kernel, dim3((unsigned)std::min<int64_t>(p.fold_items, (int64_t)1 << 22)), dim3(256), 0, st, a);
  fm->tickets.release(ticket);
  return finish_launches(s, st, hipGetLastError(), "feature mix", kWaitedLaunches);
}

// --------------------------------------------------------------------------------------
// Global feature statistics on the device (StatsAccumulator, lhotse/features/base.py:990-1033): block partials, then the fold in
// table order, in two launches (kernel_stats.hpp; the table: stats_tables.hpp)
// --------------------------------------------------------------------------------------
struct hipfeat_stats {
  int device = 0;
  int32_t feature_dim = 0;
  std::mutex mu;
  int64_t frames = 0;         // total_frames of what has been enqueued
  double* d_state = nullptr;  // [2][F]: total_sum, total_unnorm_var
  double* d_slab = nullptr;   // [blocks][2][F] of the update in flight; grows on demand
  size_t slab_cap = 0;        // bytes
  SlotRing<kTicketSlots> ring;
};

extern "C" HIPFEAT_STATS_API hipfeat_status hipfeat_stats_create(int32_t device, int32_t feature_dim, hipfeat_stats** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "stats pointer is NULL");
  *out = nullptr;
  if (feature_dim < 1 || feature_dim > kStMaxDim) return fail(HIPFEAT_ERR_INVALID, "%d bins per frame (1 ... %d)", (int)feature_dim, kStMaxDim);
  if (hipfeat_status bad = check_device(device)) return bad;
  DeviceGuard g(device);
  double* state = nullptr;
  const size_t bytes = (size_t)feature_dim * 2 * sizeof(double);
  HIP_TRY(hipMalloc(&state, bytes));
  if (hipError_t e = hipMemset(state, 0, bytes)) {
    (void)hipFree(state);
    return fail(HIPFEAT_ERR_HIP, "hipMemset failed: %s", hipGetErrorName(e));
  }
  hipfeat_stats* s = new (std::nothrow) hipfeat_stats();
  if (!s) {
    (void)hipFree(state);
    return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  }
  s->device = device;
  s->feature_dim = feature_dim;
  s->d_state = state;
  *out = s;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STATS_API hipfeat_status hipfeat_stats_destroy(hipfeat_stats* s) {
  if (!s) return HIPFEAT_OK;
  DeviceGuard g(s->device);
  s->ring.free_all();  // (waits for the launches that used a slot)
  if (s->d_slab) (void)hipFree(s->d_slab);
  if (s->d_state) (void)hipFree(s->d_state);
  delete s;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STATS_API hipfeat_status hipfeat_stats_update(hipfeat_stats* s, const void* d_feats, int64_t feats_elems, int32_t dtype, int64_t num_cuts,
                                                                 const int64_t* h_first_row, const int64_t* h_num_frames, int64_t row_stride, void* stream) {
  if (!s) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  const StPlan p = build_stats_plan(s->feature_dim, (uint64_t)reinterpret_cast<uintptr_t>(d_feats), feats_elems, dtype, num_cuts, h_first_row, h_num_frames, row_stride);
  if (p.status != 0) return fail((hipfeat_status)p.status, "%s", p.message.c_str());
  if (p.total_blocks == 0) return HIPFEAT_OK;  // cuts of no frames: nothing to add
  if (!d_feats) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)s->feature_dim, slab_bytes = (size_t)p.total_blocks * 2 * F * sizeof(double);
  if (s->slab_cap < slab_bytes) {
    // the launches that read the old slab are waited for before it goes: every update records its slot's event behind them (a failed
    // record has waited for its stream, StagedSlot::record).  The first update has no old slab and waits for nothing.
    if (s->d_slab) {
      for (auto& slot : s->ring.slots) HIP_TRY(slot.wait());
      (void)hipFree(s->d_slab);
    }
    s->d_slab = nullptr;
    s->slab_cap = 0;
    const size_t grown = std::max<size_t>(slab_bytes * 2, 1 << 20);
    HIP_TRY(hipMalloc(&s->d_slab, grown));
    s->slab_cap = grown;
  }
  StagedSlot& slot = s->ring.take();
  const size_t bytes = p.cuts.size() * sizeof(StCut);
  HIP_TRY(stage(slot, bytes, bytes, st, [&](unsigned char* h) { std::memcpy(h, p.cuts.data(), bytes); }));
  StArgs a;
  a.feats = d_feats;
  a.cuts = static_cast<const StCut*>(slot.d);
  a.slab = s->d_slab;
  a.state = s->d_state;
  a.row_stride = p.row_stride;
  a.frames_before = s->frames;
  a.num_cuts = (int32_t)p.cuts.size();
  a.feature_dim = s->feature_dim;
  a.items = (int32_t)p.items;
  a.col_tiles = (int32_t)p.col_tiles;
  a.vec_ok = p.vec_ok;
  a.pad = 0;
  if (dtype == kStF16) hipLaunchKernelGGL(stats_partial_kernel<true>, dim3(items_grid(p.items)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(stats_partial_kernel<false>, dim3(items_grid(p.items)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, st, a);
  const hipError_t e1 = hipGetLastError();
  if (e1 == hipSuccess) s->frames += p.total_frames;  // (the launches are enqueued: the state on the stream has them)
  return finish_launches(slot, st, e1, "stats", kWaitedLaunches);
}

extern "C" HIPFEAT_STATS_API hipfeat_status hipfeat_stats_merge(hipfeat_stats* s, int64_t frames, const double* h_sum, const double* h_unnorm_var, void* stream) {
  if (!s) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (frames < 0) return fail(HIPFEAT_ERR_INVALID, "a state of %lld frames", (long long)frames);
  if (frames == 0) return HIPFEAT_OK;  // an empty state adds nothing
  if (!h_sum || !h_unnorm_var) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)stream;
  const size_t F = (size_t)s->feature_dim, bytes = 2 * F * sizeof(double);
  StagedSlot& slot = s->ring.take();
  HIP_TRY(stage(slot, bytes, bytes, st, [&](unsigned char* h) {
    std::memcpy(h, h_sum, bytes / 2);
    std::memcpy(h + bytes / 2, h_unnorm_var, bytes / 2);
  }));
  hipLaunchKernelGGL(stats_merge_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, st, s->d_state, static_cast<const double*>(slot.d), (int)F, s->frames, frames);
  const hipError_t e1 = hipGetLastError();
  if (e1 == hipSuccess) s->frames += frames;
  return finish_launches(slot, st, e1, "stats merge", kWaitedLaunch);
}

extern "C" HIPFEAT_STATS_API hipfeat_status hipfeat_stats_get(hipfeat_stats* s, int64_t* h_frames, double* h_sum, double* h_unnorm_var, void* stream) {
  if (!s) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  const size_t F = (size_t)s->feature_dim;
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (h_sum) HIP_TRY(hipMemcpy(h_sum, s->d_state, F * sizeof(double), hipMemcpyDeviceToHost));
  if (h_unnorm_var) HIP_TRY(hipMemcpy(h_unnorm_var, s->d_state + F, F * sizeof(double), hipMemcpyDeviceToHost));
  if (h_frames) *h_frames = s->frames;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STATS_API hipfeat_status hipfeat_stats_reset(hipfeat_stats* s, void* stream) {
  if (!s) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  HIP_TRY(hipMemsetAsync(s->d_state, 0, (size_t)s->feature_dim * 2 * sizeof(double), (hipStream_t)stream));
  s->frames = 0;
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// Kaldi frames (Wav2Win, layers.py:151-197) and their complex STFT (Wav2FFT, layers.py:309-324) of a uniform batch: one launch of
// scalar arguments (kernel_stft.hpp)
// --------------------------------------------------------------------------------------
struct hipfeat_stft {
  StftFront front;
  int device = 0;
  const void* fn = nullptr;
  const void* fn_ragged = nullptr;  // the same body on RaggedRowSource
  std::mutex mu;                    // hipfeat_stft_run_ragged: the ring of its length tables
  SlotRing<4> ring;
};

// The length table of a ragged call (kernel_stft.hpp, RaggedArgs): rows x {S_b, T_b}.  Checks the lengths against max_samples and the
// reflection, names the offending row, and yields Tmax; touches no device.
static hipfeat_status ragged_table(const int64_t* h_lengths, int64_t batch, int64_t max_samples, int N, int shift, bool snip, std::vector<int64_t>& table,
                                   int64_t* tmax) {
  table.resize((size_t)batch * 2);
  *tmax = 0;
  for (int64_t b = 0; b < batch; ++b) {
    const int64_t S = h_lengths[b];
    if (S < 0 || S > max_samples)
      return fail(HIPFEAT_ERR_INVALID, "row %lld: length %lld is outside [0, max_samples = %lld]", (long long)b, (long long)S, (long long)max_samples);
    if (hipfeat_status bad = hipfeat_check_length(S, N, shift, snip)) {
      const std::string why = g_err;
      return fail(bad, "row %lld: %s", (long long)b, why.c_str());
    }
    const int64_t T = hipfeat_num_frames(S, N, shift, snip);
    table[(size_t)(2 * b)] = S, table[(size_t)(2 * b + 1)] = T;
    *tmax = std::max(*tmax, T);
  }
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STFT_API hipfeat_status hipfeat_stft_destroy(hipfeat_stft* s) {
  if (!s) return HIPFEAT_OK;
  DeviceGuard g(s->device);
  s->ring.free_all();  // (waits for the launches that used a slot)
  stft_front_free(s->front);
  delete s;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STFT_API hipfeat_status hipfeat_stft_create(const hipfeat_stft_config* cfg, const float* h_window, int32_t device, hipfeat_stft** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "stft pointer is NULL");
  *out = nullptr;
  int n1 = 0;
  if (hipfeat_status bad = check_stft_config(cfg, h_window, false, &n1)) return bad;
  if (hipfeat_status bad = require_gfx950(device)) return bad;
  hipfeat_stft* s = new (std::nothrow) hipfeat_stft();
  if (!s) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  s->device = device;
  const bool spectrum = cfg->output == HIPFEAT_STFT_SPECTRUM;
  s->fn = for_n1(n1, [&](auto n) { return spectrum ? entry<stft_kernel<decltype(n)::value, 1>>() : entry<stft_kernel<decltype(n)::value, 0>>(); });
  s->fn_ragged = for_n1(n1, [&](auto n) { return spectrum ? entry<stft_ragged_kernel<decltype(n)::value, 1>>() : entry<stft_ragged_kernel<decltype(n)::value, 0>>(); });
  DeviceGuard g(device);
  hipfeat_status bad = stft_front_create(s->front, *cfg, n1, h_window, s->fn);
  if (bad == HIPFEAT_OK) bad = set_dynamic_lds(s->fn_ragged, s->front.lds);
  if (bad != HIPFEAT_OK) {
    hipfeat_stft_destroy(s);
    return bad;
  }
  *out = s;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STFT_API hipfeat_status hipfeat_stft_run(hipfeat_stft* s, const float* d_wave, int64_t batch, int64_t num_samples, int64_t row_stride,
                                                            float* d_out, int64_t out_floats, float* d_log_energy, void* stream) {
  if (!s) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  const hipfeat_stft_config& c = s->front.cfg;
  if (batch < 0 || num_samples < 0 || out_floats < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  if (batch > 1 && row_stride < num_samples) return fail(HIPFEAT_ERR_INVALID, "row_stride = %lld < num_samples = %lld", (long long)row_stride, (long long)num_samples);
  const int64_t T = hipfeat_num_frames(num_samples, c.frame_length, c.frame_shift, c.snip_edges);
  if (batch == 0) return HIPFEAT_OK;
  // (without snip_edges a row of no frames is too short as well, as for the feature plans)
  if (hipfeat_status bad = hipfeat_check_length(num_samples, c.frame_length, c.frame_shift, c.snip_edges)) return bad;
  if (T == 0) return HIPFEAT_OK;
  const int64_t width = s->front.width();
  if (batch > INT64_MAX / T || batch * T > INT64_MAX / width) return fail(HIPFEAT_ERR_INVALID, "%lld x %lld frames overflow", (long long)batch, (long long)T);
  if (out_floats < batch * T * width)
    return fail(HIPFEAT_ERR_INVALID, "output of %lld floats, %lld x %lld x %lld needed", (long long)out_floats, (long long)batch, (long long)T, (long long)width);
  if (!d_wave || !d_out) return fail(HIPFEAT_ERR_INVALID, "NULL device pointer");
  const int align = s->front.spectrum() ? 8 : 4;
  if (reinterpret_cast<uintptr_t>(d_wave) % 4 || reinterpret_cast<uintptr_t>(d_out) % align || reinterpret_cast<uintptr_t>(d_log_energy) % 4)
    return fail(HIPFEAT_ERR_INVALID, "misaligned device pointer (samples and log-energies: 4 bytes, output: %d)", align);
  const int64_t fpb = 4 * kStftFramesPerWave, bpr = (T + fpb - 1) / fpb;
  if (bpr > INT32_MAX / batch) return fail(HIPFEAT_ERR_UNSUPPORTED, "%lld workgroups in one launch", (long long)batch * (long long)bpr);
  StftParams p{};
  fill_stft_front(p, s->front);
  p.wave = d_wave;
  p.out = d_out;
  p.log_energy = c.want_energy ? d_log_energy : nullptr;
  p.row_stride = row_stride;
  p.num_samples = num_samples;
  p.frames_per_row = T;
  p.blocks_per_row = bpr;
  p.npad_left = c.snip_edges ? 0 : (c.frame_length - c.frame_shift) / 2;
  void* args[] = {&p};
  DeviceGuard g(s->device);
  set_lds_poison(s->front.lds);
  (void)hipLaunchKernel(s->fn, dim3((unsigned)(batch * bpr)), dim3(256), args, s->front.lds, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return HIPFEAT_OK;
}

// ... of a zero-padded batch whose row b holds h_lengths[b] samples: the same body on RaggedRowSource, the padding rows of the
// (batch, Tmax, width) output written by the same launch; the length table travels through a slot of the handle's ring
extern "C" HIPFEAT_RAGGED_API hipfeat_status hipfeat_stft_run_ragged(hipfeat_stft* s, const float* d_wave, int64_t batch, int64_t max_samples, int64_t row_stride,
                                                                   const int64_t* h_lengths, float padding_value, float* d_out, int64_t out_floats,
                                                                   float* d_log_energy, void* stream) {
  if (!s) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  const hipfeat_stft_config& c = s->front.cfg;
  if (batch < 0 || max_samples < 0 || out_floats < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  if (batch > 0 && !h_lengths) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (batch > 1 && row_stride < max_samples) return fail(HIPFEAT_ERR_INVALID, "row_stride = %lld < max_samples = %lld", (long long)row_stride, (long long)max_samples);
  std::vector<int64_t> table;
  int64_t T = 0;  // Tmax
  if (hipfeat_status bad = ragged_table(h_lengths, batch, max_samples, c.frame_length, c.frame_shift, c.snip_edges != 0, table, &T)) return bad;
  if (batch == 0 || T == 0) return HIPFEAT_OK;  // (no frame, no padding row: nothing to write)
  const int64_t width = s->front.width();
  if (batch > INT64_MAX / T || batch * T > INT64_MAX / width) return fail(HIPFEAT_ERR_INVALID, "%lld x %lld frames overflow", (long long)batch, (long long)T);
  if (out_floats < batch * T * width)
    return fail(HIPFEAT_ERR_INVALID, "output of %lld floats, %lld x %lld x %lld needed", (long long)out_floats, (long long)batch, (long long)T, (long long)width);
  if (!d_wave || !d_out) return fail(HIPFEAT_ERR_INVALID, "NULL device pointer");
  const int align = s->front.spectrum() ? 8 : 4;
  if (reinterpret_cast<uintptr_t>(d_wave) % 4 || reinterpret_cast<uintptr_t>(d_out) % align || reinterpret_cast<uintptr_t>(d_log_energy) % 4)
    return fail(HIPFEAT_ERR_INVALID, "misaligned device pointer (samples and log-energies: 4 bytes, output: %d)", align);
  const int64_t fpb = 4 * kStftFramesPerWave, bpr = (T + fpb - 1) / fpb;
  if (bpr > INT32_MAX / batch) return fail(HIPFEAT_ERR_UNSUPPORTED, "%lld workgroups in one launch", (long long)batch * (long long)bpr);
  StftParams p{};
  fill_stft_front(p, s->front);
  p.wave = d_wave;
  p.out = d_out;
  p.log_energy = c.want_energy ? d_log_energy : nullptr;
  p.row_stride = row_stride;
  p.num_samples = max_samples;
  p.frames_per_row = T;
  p.blocks_per_row = bpr;
  p.npad_left = c.snip_edges ? 0 : (c.frame_length - c.frame_shift) / 2;
  std::lock_guard<std::mutex> lk(s->mu);
  DeviceGuard g(s->device);
  hipStream_t st = (hipStream_t)stream;
  StagedSlot& slot = s->ring.take();
  const size_t bytes = table.size() * sizeof(int64_t);
  HIP_TRY(stage(slot, bytes, bytes, st, [&](unsigned char* h) { std::memcpy(h, table.data(), bytes); }));
  RaggedArgs a{static_cast<const int64_t*>(slot.d), padding_value};
  void* args[] = {&p, &a};
  set_lds_poison(s->front.lds);
  (void)hipLaunchKernel(s->fn_ragged, dim3((unsigned)(batch * bpr)), dim3(256), args, s->front.lds, st);
  return finish_launches(slot, st, hipGetLastError(), "ragged stft", kWaitedLaunch);
}

// --------------------------------------------------------------------------------------
// Streaming layers (online_inference, layers.py:199-224, 326-333, 775-856): one launch frames V = [context | chunk], computes what
// `forward` computes per frame and writes the remainder (kernel_stream.hpp)
// --------------------------------------------------------------------------------------
struct hipfeat_stream {
  int device = 0;
  const void* fn = nullptr;
  bool features = false;
  StftFront front;        // frames / spectrum: the STFT front end on the two-span source
  hipfeat_config fcfg{};  // features: the wave kernel on tables of its own (`uploads`), its Params complete but for the call's buffers
  WaveParams wave{};
  size_t wave_lds = 0;
  std::vector<void*> uploads;
};

extern "C" HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_destroy(hipfeat_stream* s) {
  if (!s) return HIPFEAT_OK;
  DeviceGuard g(s->device);
  stft_front_free(s->front);
  free_uploads(s->uploads);
  delete s;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_counts(int32_t frame_length, int32_t frame_shift, int32_t snip_edges, int32_t first,
                                                                   int64_t context_len, int64_t chunk_len, int64_t* frames, int64_t* remainder_len) {
  if (!frames || !remainder_len) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  *frames = *remainder_len = 0;
  if (frame_length <= 0 || frame_shift <= 0)
    return fail(HIPFEAT_ERR_INVALID, "frame_length = %d, frame_shift = %d: both must be positive", (int)frame_length, (int)frame_shift);
  if (context_len < 0 || chunk_len < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  if (first && context_len != 0) return fail(HIPFEAT_ERR_INVALID, "the first call of a stream has no context, context_len = %lld", (long long)context_len);
  if (frame_shift > frame_length) return fail(HIPFEAT_ERR_UNSUPPORTED, "frame_shift (%d) > frame_length (%d) is not supported", (int)frame_shift, (int)frame_length);
  const int64_t head = first ? (snip_edges ? 0 : std::min<int64_t>((frame_length - frame_shift) / 2, chunk_len)) : context_len;
  if (head > INT64_MAX - chunk_len) return fail(HIPFEAT_ERR_INVALID, "%lld + %lld samples overflow", (long long)head, (long long)chunk_len);
  const int64_t L = head + chunk_len;
  const int64_t T = L < frame_length ? 0 : 1 + (L - frame_length) / frame_shift;
  *frames = T;
  *remainder_len = L - T * frame_shift;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_create_features(const hipfeat_config* cfg, const float* h_window, const float* h_mel,
                                                                            const float* h_dct, const float* h_lifter, int32_t device, hipfeat_stream** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "stream pointer is NULL");
  *out = nullptr;
  if (!cfg) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (hipfeat_status bad = check_feature_config(cfg, h_window, h_mel, h_dct, h_lifter)) return bad;
  const int N = cfg->frame_length, shift = cfg->frame_shift, fft = cfg->fft_length;
  if (cfg->kind > HIPFEAT_MFCC) return fail(HIPFEAT_ERR_UNSUPPORTED, "kind %d: the streaming kernel has the four Kaldi layer kinds (spectrogram, log-spectrogram, fbank, mfcc)", (int)cfg->kind);
  if (!radix_fft_size(fft))
    return fail(HIPFEAT_ERR_UNSUPPORTED, "fft_length = %d: the streaming kernel has the sizes 256, 512, 1024 and 2048 (round_to_power_of_two=True, 8 to 48 kHz at 25 ms)", fft);
  const bool need_mel = cfg->kind >= HIPFEAT_FBANK;
  if (need_mel && cfg->num_filters > 128) return fail(HIPFEAT_ERR_UNSUPPORTED, "num_filters = %d: the streaming kernel holds at most 128 filters", (int)cfg->num_filters);
  const int M = need_mel ? cfg->num_filters : 0, C = cfg->kind == HIPFEAT_MFCC ? cfg->num_ceps : 0;
  // the wave kernel's own tables (plan_tables.hpp), not a plan's: a plan's tables are those of the instance it picked
  PlanInputs in;
  in.N = N, in.shift = shift, in.K = fft / 2 + 1, in.M = M, in.C = C;
  in.window = h_window, in.mel = h_mel, in.dct = h_dct, in.lifter = cfg->apply_lifter ? h_lifter : nullptr;
  const WaveTables t = build_wave_tables(in, fft / 2);
  if (t.lds > 160 * 1024) return fail(HIPFEAT_ERR_UNSUPPORTED, "configuration does not fit in LDS (%zu bytes)", t.lds);
  if (hipfeat_status bad = require_gfx950(device)) return bad;
  DeviceGuard g(device);
  hipfeat_stream* s = new (std::nothrow) hipfeat_stream();
  if (!s) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  s->features = true;
  s->fcfg = *cfg;
  s->device = device;
  s->fn = for_n1(fft / 128, [](auto n) { return entry<wave_stream_kernel<decltype(n)::value>>(); });
  WaveParams& w = s->wave;
  fill_wave_front(w, *cfg, t);
  w.frames_per_wave = kStftFramesPerWave;  // (npad_left stays 0: V starts at its first frame)
  s->wave_lds = t.lds;
  const std::vector<float2> tw = fft_twiddles(fft, fft / 2);
  hipfeat_status st = upload(s->uploads, w.window, h_window, (size_t)N);
  if (st == HIPFEAT_OK) st = upload(s->uploads, w.tw, tw.data(), tw.size());
  if (st == HIPFEAT_OK && M > 0) st = upload(s->uploads, w.mel_blob, t.blob.data(), t.blob.size());
  if (st == HIPFEAT_OK && C > 0) st = upload(s->uploads, w.dct, h_dct, (size_t)M * C);
  if (st == HIPFEAT_OK && C > 0 && cfg->apply_lifter) st = upload(s->uploads, w.lifter, h_lifter, (size_t)C);
  if (st == HIPFEAT_OK) st = set_dynamic_lds(s->fn, s->wave_lds);
  if (st != HIPFEAT_OK) {
    hipfeat_stream_destroy(s);
    return st;
  }
  *out = s;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_create_stft(const hipfeat_stft_config* cfg, const float* h_window, int32_t device, hipfeat_stream** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "stream pointer is NULL");
  *out = nullptr;
  int n1 = 0;
  if (hipfeat_status bad = check_stft_config(cfg, h_window, true, &n1)) return bad;
  if (hipfeat_status bad = require_gfx950(device)) return bad;
  hipfeat_stream* s = new (std::nothrow) hipfeat_stream();
  if (!s) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  s->device = device;
  const bool spectrum = cfg->output == HIPFEAT_STFT_SPECTRUM;
  s->fn = for_n1(n1, [&](auto n) { return spectrum ? entry<stft_stream_kernel<decltype(n)::value, 1>>() : entry<stft_stream_kernel<decltype(n)::value, 0>>(); });
  DeviceGuard g(device);
  if (hipfeat_status bad = stft_front_create(s->front, *cfg, n1, h_window, s->fn)) {
    hipfeat_stream_destroy(s);
    return bad;
  }
  *out = s;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_STREAM_API hipfeat_status hipfeat_stream_run(hipfeat_stream* s, const float* d_context, int64_t context_len, int64_t context_stride,
                                                                const float* d_chunk, int64_t chunk_len, int64_t chunk_stride, int64_t batch, float* d_out,
                                                                int64_t out_floats, float* d_log_energy, float* d_remainder, int64_t remainder_floats,
                                                                void* stream) {
  if (!s) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (batch < 0 || context_len < 0 || chunk_len < 0 || out_floats < 0 || remainder_floats < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  const bool first = d_context == nullptr;
  if (first && context_len != 0) return fail(HIPFEAT_ERR_INVALID, "NULL context with context_len = %lld", (long long)context_len);
  if (batch > 1 && (chunk_stride < chunk_len || (!first && context_stride < context_len)))
    return fail(HIPFEAT_ERR_INVALID, "a row stride is shorter than its row (context %lld < %lld or chunk %lld < %lld)", (long long)context_stride, (long long)context_len,
                (long long)chunk_stride, (long long)chunk_len);
  const hipfeat_config& fc = s->fcfg;
  const hipfeat_stft_config& sc = s->front.cfg;
  const int N = s->features ? fc.frame_length : sc.frame_length, shift = s->features ? fc.frame_shift : sc.frame_shift;
  const bool snip = (s->features ? fc.snip_edges : sc.snip_edges) != 0;
  int64_t T = 0, rem = 0;
  if (hipfeat_status bad = hipfeat_stream_counts(N, shift, snip ? 1 : 0, first ? 1 : 0, context_len, chunk_len, &T, &rem)) return bad;
  if (batch == 0) return HIPFEAT_OK;
  const int64_t width = s->features ? feature_dim(fc) : s->front.width();
  if (T > INT32_MAX || (T > 0 && (batch > INT64_MAX / T || batch * T > INT64_MAX / width)) || (rem > 0 && batch > INT64_MAX / rem))
    return fail(HIPFEAT_ERR_INVALID, "%lld x %lld frames overflow", (long long)batch, (long long)T);
  if (out_floats < batch * T * width)
    return fail(HIPFEAT_ERR_INVALID, "output of %lld floats, %lld x %lld x %lld needed", (long long)out_floats, (long long)batch, (long long)T, (long long)width);
  if (remainder_floats < batch * rem)
    return fail(HIPFEAT_ERR_INVALID, "remainder of %lld floats, %lld x %lld needed", (long long)remainder_floats, (long long)batch, (long long)rem);
  if ((chunk_len > 0 && !d_chunk) || (T > 0 && !d_out) || (rem > 0 && !d_remainder)) return fail(HIPFEAT_ERR_INVALID, "NULL device pointer");
  const int align = !s->features && s->front.spectrum() ? 8 : 4;
  if (reinterpret_cast<uintptr_t>(d_context) % 4 || reinterpret_cast<uintptr_t>(d_chunk) % 4 || reinterpret_cast<uintptr_t>(d_out) % align ||
      reinterpret_cast<uintptr_t>(d_log_energy) % 4 || reinterpret_cast<uintptr_t>(d_remainder) % 4)
    return fail(HIPFEAT_ERR_INVALID, "misaligned device pointer (samples, log-energies and remainder: 4 bytes, output: %d)", align);
  if (T == 0 && rem == 0) return HIPFEAT_OK;  // nothing to frame and nothing to hand back
  const int64_t fpb = 4 * kStftFramesPerWave, bpr = std::max<int64_t>((T + fpb - 1) / fpb, 1);
  if (bpr > INT32_MAX / batch) return fail(HIPFEAT_ERR_UNSUPPORTED, "%lld workgroups in one launch", (long long)batch * (long long)bpr);
  StreamArgs a{};
  a.ctx = d_context;
  a.chunk = d_chunk;
  a.remainder = d_remainder;
  a.ctx_stride = context_stride;
  a.chunk_stride = chunk_stride;
  a.flipped = first && !snip ? 1 : 0;
  a.R = first ? (snip ? 0 : std::min<int64_t>((N - shift) / 2, chunk_len)) : context_len;
  a.S = chunk_len;
  a.T = T;
  a.blocks_per_row = bpr;
  a.shift = shift;
  // the params of either kernel; npad_left stays 0: V starts at its first frame
  WaveParams wp = s->wave;
  StftParams sp{};
  void* args[] = {nullptr, &a};
  if (s->features) {
    wp.out = d_out;
    wp.out_stride = width;
    args[0] = &wp;
  } else {
    fill_stft_front(sp, s->front);
    sp.out = d_out;
    sp.log_energy = (sc.want_energy && !s->front.spectrum()) ? d_log_energy : nullptr;  // (the spectrum carries it in bin 0)
    sp.frames_per_row = T;
    sp.blocks_per_row = bpr;
    args[0] = &sp;
  }
  const size_t lds = s->features ? s->wave_lds : s->front.lds;
  DeviceGuard g(s->device);
  set_lds_poison(lds);
  (void)hipLaunchKernel(s->fn, dim3((unsigned)(batch * bpr)), dim3(256), args, lds, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return HIPFEAT_OK;
}

// --------------------------------------------------------------------------------------
// Waveform gradient of the six layers (the autograd of layers.py): per piece of rows one launch that writes every frame's sbar into the
// caller's workspace and one that gathers it into the waveform's gradient (kernel_grad.hpp, grad_tables.hpp)
// --------------------------------------------------------------------------------------
struct hipfeat_grad {
  int device = 0;
  const void* fn = nullptr;
  int mode = 0, n1 = 0, N = 0, shift = 0, fft = 0, M = 0, C = 0, width = 0, flags = 0;
  bool snip = false, energy_rows = false, blob_in_lds = false;
  float preemph = 0.f, log_floor = 0.f, mel_floor = 0.f, log_offset = 0.f;
  size_t lds = 0, off_tw = 0, off_tw64 = 0, off_blob = 0;  // bytes into the slot
  int blob_floats = 0, off_fwd = 0, off_bwd = 0, off_dct = 0, off_lifter = 0;
  StagedSlot slot;  // device: [window | W_fft^k | W_fft^k in float64 | filterbank blob], staged once at creation
  const void* fn_ragged = nullptr;  // the same body on RaggedRowSource
  std::mutex mu;                    // hipfeat_grad_run_ragged: the ring of its length tables
  SlotRing<4> ring;
};

extern "C" HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_destroy(hipfeat_grad* g) {
  if (!g) return HIPFEAT_OK;
  DeviceGuard guard(g->device);
  g->ring.free_all();  // (waits for the launches that used a slot)
  g->slot.free_all();
  delete g;
  return HIPFEAT_OK;
}

// the checked handle `g` on `device`: the kernel instance, its LDS, and the tables through the handle's slot
static hipfeat_status grad_finish_create(hipfeat_grad* g, int32_t device, const float* h_window, const GradTables& t, hipfeat_grad** out) {
  const bool spectral = g->mode != GRAD_FRAMES;
  g->device = device;
  g->fn = for_n1(g->n1, [](auto n) { return entry<grad_frames_kernel<decltype(n)::value>>(); });
  g->fn_ragged = for_n1(g->n1, [](auto n) { return entry<grad_frames_ragged_kernel<decltype(n)::value>>(); });
  g->blob_floats = (int)t.blob.size();
  g->off_fwd = t.off_fwd, g->off_bwd = t.off_bwd, g->off_dct = t.off_dct, g->off_lifter = t.off_lifter;
  g->blob_in_lds = g->blob_floats > 0 && grad_blob_fits_lds(g->n1, g->N, t.blob.size());
  g->lds = sizeof(float) * (grad_lds_floats(g->n1, g->N) + (g->blob_in_lds ? t.blob.size() : 0));
  const size_t win_bytes = sizeof(float) * (size_t)((g->N + 3) & ~3), tw_bytes = spectral ? sizeof(float2) * (size_t)(g->fft / 2) : 0;
  g->off_tw = win_bytes;
  g->off_tw64 = (win_bytes + tw_bytes + 15) & ~(size_t)15;
  std::vector<double> tw64;  // (re, im) of W_fft^k, k < fft / 2: the recomputed spectrum of the feature kinds runs in float64
  if (g->mode <= GRAD_MFCC)
    for (int k = 0; k < g->fft / 2; ++k) {
      const double a = -2.0 * M_PI * (double)k / (double)g->fft;
      tw64.push_back(std::cos(a)), tw64.push_back(std::sin(a));
    }
  g->off_blob = g->off_tw64 + sizeof(double) * tw64.size();
  const size_t total = g->off_blob + sizeof(float) * t.blob.size();
  const std::vector<float2> tw = spectral ? fft_twiddles(g->fft, g->fft / 2) : std::vector<float2>();
  DeviceGuard guard(device);
  hipError_t e = stage(g->slot, total, total, nullptr, [&](unsigned char* h) {
    std::memset(h, 0, total);
    std::memcpy(h, h_window, sizeof(float) * (size_t)g->N);
    if (!tw.empty()) std::memcpy(h + g->off_tw, tw.data(), tw_bytes);
    if (!tw64.empty()) std::memcpy(h + g->off_tw64, tw64.data(), sizeof(double) * tw64.size());
    if (!t.blob.empty()) std::memcpy(h + g->off_blob, t.blob.data(), sizeof(float) * t.blob.size());
  });
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  hipfeat_status st = e == hipSuccess ? HIPFEAT_OK : fail(HIPFEAT_ERR_HIP, "staging the gradient tables failed: %s", hipGetErrorName(e));
  if (st == HIPFEAT_OK) st = set_dynamic_lds(g->fn, g->lds);
  if (st == HIPFEAT_OK) st = set_dynamic_lds(g->fn_ragged, g->lds);
  if (st != HIPFEAT_OK) {
    hipfeat_grad_destroy(g);
    return st;
  }
  *out = g;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_create_features(const hipfeat_config* cfg, const float* h_window, const float* h_mel, const float* h_dct,
                                                                        const float* h_lifter, int32_t device, hipfeat_grad** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "grad pointer is NULL");
  *out = nullptr;
  if (!cfg) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (hipfeat_status bad = check_feature_config(cfg, h_window, h_mel, h_dct, h_lifter)) return bad;
  const int fft = cfg->fft_length;
  if (cfg->kind > HIPFEAT_MFCC) return fail(HIPFEAT_ERR_UNSUPPORTED, "kind %d: the gradient kernel has the four Kaldi layer kinds (spectrogram, log-spectrogram, fbank, mfcc)", (int)cfg->kind);
  if (!radix_fft_size(fft))
    return fail(HIPFEAT_ERR_UNSUPPORTED, "fft_length = %d: the gradient kernel has the sizes 256, 512, 1024 and 2048 (round_to_power_of_two=True, 8 to 48 kHz at 25 ms)", fft);
  const bool need_mel = cfg->kind >= HIPFEAT_FBANK;
  if (need_mel && cfg->num_filters > 128) return fail(HIPFEAT_ERR_UNSUPPORTED, "num_filters = %d: the gradient kernel holds at most 128 filters", (int)cfg->num_filters);
  const int M = need_mel ? cfg->num_filters : 0, C = cfg->kind == HIPFEAT_MFCC ? cfg->num_ceps : 0;
  const GradTables t = build_grad_tables(fft / 2 + 1, M, C, h_mel, h_dct, cfg->apply_lifter ? h_lifter : nullptr);
  if (hipfeat_status bad = require_gfx950(device)) return bad;
  hipfeat_grad* g = new (std::nothrow) hipfeat_grad();
  if (!g) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  g->mode = cfg->kind;
  g->n1 = fft / 128;
  g->N = cfg->frame_length, g->shift = cfg->frame_shift, g->fft = fft, g->M = M, g->C = C;
  g->width = feature_dim(*cfg);
  g->flags = energy_flags(*cfg);
  g->snip = cfg->snip_edges != 0;
  g->preemph = cfg->preemph_coeff;
  g->log_floor = log_energy_floor(cfg->energy_floor);
  g->mel_floor = cfg->mel_floor;
  g->log_offset = cfg->log_offset;
  return grad_finish_create(g, device, h_window, t, out);
}

extern "C" HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_create_stft(const hipfeat_stft_config* cfg, const float* h_window, int32_t device, hipfeat_grad** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "grad pointer is NULL");
  *out = nullptr;
  int n1 = 0;
  if (hipfeat_status bad = check_stft_config(cfg, h_window, true, &n1)) return bad;
  if (hipfeat_status bad = require_gfx950(device)) return bad;
  hipfeat_grad* g = new (std::nothrow) hipfeat_grad();
  if (!g) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  const bool spectrum = cfg->output == HIPFEAT_STFT_SPECTRUM;
  g->mode = spectrum ? GRAD_SPECTRUM : GRAD_FRAMES;
  g->n1 = n1;
  g->N = cfg->frame_length, g->shift = cfg->frame_shift, g->fft = cfg->pad_length;
  g->width = cfg->pad_length + (spectrum ? 2 : 0);
  g->flags = energy_flags(*cfg);
  g->snip = cfg->snip_edges != 0;
  g->energy_rows = cfg->want_energy && !spectrum;
  g->preemph = cfg->preemph_coeff;
  g->log_floor = log_energy_floor(cfg->energy_floor);
  return grad_finish_create(g, device, h_window, GradTables(), out);
}

// The arguments of the two launches of a piece but for the piece's own pointers and row count, for rows of `num_samples` samples and T
// frames (a ragged batch: Smax and Tmax), common to hipfeat_grad_run and hipfeat_grad_run_ragged
static void fill_grad_params(const hipfeat_grad* g, const GradPieces& pc, int64_t num_samples, int64_t T, int64_t row_stride, int64_t grad_wave_stride,
                             float* d_workspace, int64_t bpr, int64_t gpr, GradParams& p, GradOlaParams& o) {
  const unsigned char* tables = static_cast<const unsigned char*>(g->slot.d);
  p.window = reinterpret_cast<const float*>(tables);
  p.tw = g->mode == GRAD_FRAMES ? nullptr : reinterpret_cast<const float2*>(tables + g->off_tw);
  p.tw64 = g->mode <= GRAD_MFCC ? reinterpret_cast<const double2*>(tables + g->off_tw64) : nullptr;
  p.blob = g->blob_floats ? reinterpret_cast<const float*>(tables + g->off_blob) : nullptr;
  p.ws = d_workspace;
  p.row_stride = row_stride, p.num_samples = num_samples, p.frames_per_row = T, p.blocks_per_row = bpr, p.width = g->width;
  p.N = g->N, p.Nr = (int32_t)pc.Nr, p.shift = g->shift, p.npad_left = g->snip ? 0 : (g->N - g->shift) / 2;
  p.frames_per_wave = kStftFramesPerWave, p.flags = g->flags, p.mode = g->mode;
  p.M = g->M, p.C = g->C, p.blob_floats = g->blob_floats, p.blob_in_lds = g->blob_in_lds ? 1 : 0;
  p.off_fwd = g->off_fwd, p.off_bwd = g->off_bwd, p.off_dct = g->off_dct, p.off_lifter = g->off_lifter;
  p.preemph = g->preemph, p.log_energy_floor = g->log_floor, p.mel_floor = g->mel_floor, p.log_offset = g->log_offset;
  o.ws = d_workspace;
  o.S = num_samples, o.T = T, o.groups_per_row = gpr, o.stride = grad_wave_stride;
  o.N = g->N, o.Nr = (int32_t)pc.Nr, o.shift = g->shift, o.npad_left = p.npad_left;
}

extern "C" HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_workspace(const hipfeat_grad* g, int64_t batch, int64_t num_samples, int64_t budget_bytes,
                                                                  int64_t* rows_per_piece, int64_t* floats) {
  if (!g || !rows_per_piece || !floats) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  *rows_per_piece = *floats = 0;
  if (batch < 0 || num_samples < 0 || budget_bytes < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  GradPieces pc;
  if (!grad_pieces(batch, hipfeat_num_frames(num_samples, g->N, g->shift, g->snip), g->N, budget_bytes, &pc))
    return fail(HIPFEAT_ERR_INVALID, "%lld rows of %lld samples overflow", (long long)batch, (long long)num_samples);
  *rows_per_piece = pc.rows_per_piece;
  *floats = pc.floats;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_GRAD_API hipfeat_status hipfeat_grad_run(hipfeat_grad* g, const float* d_wave, int64_t batch, int64_t num_samples, int64_t row_stride,
                                                            const float* d_grad_out, int64_t grad_out_floats, const float* d_grad_log_energy, float* d_grad_wave,
                                                            int64_t grad_wave_stride, float* d_workspace, int64_t workspace_floats, void* stream) {
  if (!g) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (batch < 0 || num_samples < 0 || grad_out_floats < 0 || workspace_floats < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  if (batch > 1 && (row_stride < num_samples || grad_wave_stride < num_samples))
    return fail(HIPFEAT_ERR_INVALID, "a row stride is shorter than its row (waveform %lld, gradient %lld, num_samples = %lld)", (long long)row_stride,
                (long long)grad_wave_stride, (long long)num_samples);
  const int64_t T = hipfeat_num_frames(num_samples, g->N, g->shift, g->snip);
  if (batch == 0) return HIPFEAT_OK;
  if (hipfeat_status bad = hipfeat_check_length(num_samples, g->N, g->shift, g->snip)) return bad;
  if (num_samples == 0) return HIPFEAT_OK;
  GradPieces pc;
  if (!grad_pieces(batch, T, g->N, 0, &pc) || (T > 0 && batch > INT64_MAX / T / g->width))
    return fail(HIPFEAT_ERR_INVALID, "%lld x %lld frames overflow", (long long)batch, (long long)T);
  const bool frames_mode = g->mode == GRAD_FRAMES;
  if (!d_grad_out && !frames_mode) return fail(HIPFEAT_ERR_INVALID, "NULL device pointer (only a frames handle takes a NULL output cotangent)");
  if (d_grad_out && grad_out_floats < batch * T * g->width)
    return fail(HIPFEAT_ERR_INVALID, "output cotangent of %lld floats, %lld x %lld x %lld needed", (long long)grad_out_floats, (long long)batch, (long long)T,
                (long long)g->width);
  if (!d_wave || !d_grad_wave) return fail(HIPFEAT_ERR_INVALID, "NULL device pointer");
  if (T > 0 && (!d_workspace || workspace_floats < pc.row_floats))
    return fail(HIPFEAT_ERR_INVALID, "workspace of %lld floats, one row of %lld frames needs %lld", (long long)workspace_floats, (long long)T, (long long)pc.row_floats);
  if (reinterpret_cast<uintptr_t>(d_wave) % 4 || reinterpret_cast<uintptr_t>(d_grad_out) % 4 || reinterpret_cast<uintptr_t>(d_grad_log_energy) % 4 ||
      reinterpret_cast<uintptr_t>(d_grad_wave) % 4 || reinterpret_cast<uintptr_t>(d_workspace) % 16)
    return fail(HIPFEAT_ERR_INVALID, "misaligned device pointer (samples, cotangents and gradient: 4 bytes, workspace: 16)");
  const int64_t fpb = 4 * kStftFramesPerWave, bpr = (T + fpb - 1) / fpb, gpr = (num_samples + 3) / 4 + 1;
  if (bpr > INT32_MAX || gpr > (int64_t)INT32_MAX * 128) return fail(HIPFEAT_ERR_UNSUPPORTED, "a row of %lld samples is too long for one launch", (long long)num_samples);
  int64_t rpp = T > 0 ? workspace_floats / pc.row_floats : batch;
  rpp = std::min({rpp, batch, T > 0 ? INT32_MAX / bpr : batch, (int64_t)INT32_MAX * 128 / gpr});
  GradParams p{};
  GradOlaParams o{};
  fill_grad_params(g, pc, num_samples, T, row_stride, grad_wave_stride, d_workspace, bpr, gpr, p, o);
  DeviceGuard guard(g->device);
  set_lds_poison(g->lds);
  for (int64_t r0 = 0; r0 < batch; r0 += rpp) {
    const int64_t rows = std::min(rpp, batch - r0);
    p.wave = d_wave + r0 * row_stride;
    p.gout = d_grad_out ? d_grad_out + r0 * T * g->width : nullptr;
    p.glog_e = (g->energy_rows && d_grad_log_energy) ? d_grad_log_energy + r0 * T : nullptr;
    o.gwave = d_grad_wave + r0 * grad_wave_stride;
    o.rows = rows;
    void* pa[] = {&p};
    void* oa[] = {&o};
    if (T > 0) (void)hipLaunchKernel(g->fn, dim3((unsigned)(rows * bpr)), dim3(256), pa, g->lds, (hipStream_t)stream);
    (void)hipLaunchKernel(reinterpret_cast<const void*>(grad_overlap_add_kernel), dim3((unsigned)((rows * gpr + 255) / 256)), dim3(256), oa, 0, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
  }
  return HIPFEAT_OK;
}

// ... of a zero-padded batch whose row b holds h_lengths[b] samples: the piece arithmetic at Tmax = max_b T_b (the workspace stays dense)
extern "C" HIPFEAT_RAGGED_API hipfeat_status hipfeat_grad_workspace_ragged(const hipfeat_grad* g, int64_t batch, int64_t max_samples, const int64_t* h_lengths,
                                                                         int64_t budget_bytes, int64_t* rows_per_piece, int64_t* floats) {
  if (!g || !rows_per_piece || !floats || (batch > 0 && !h_lengths)) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  *rows_per_piece = *floats = 0;
  if (batch < 0 || max_samples < 0 || budget_bytes < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  std::vector<int64_t> table;
  int64_t T = 0;
  if (hipfeat_status bad = ragged_table(h_lengths, batch, max_samples, g->N, g->shift, g->snip, table, &T)) return bad;
  GradPieces pc;
  if (!grad_pieces(batch, T, g->N, budget_bytes, &pc)) return fail(HIPFEAT_ERR_INVALID, "%lld rows of %lld samples overflow", (long long)batch, (long long)max_samples);
  *rows_per_piece = pc.rows_per_piece;
  *floats = pc.floats;
  return HIPFEAT_OK;
}

// ... the two launches per piece on RaggedRowSource and the row's own index map; the cotangent (batch, Tmax, row) and the gradient
// (batch, max_samples) are those of the ragged forward, the length table travels through a slot of the handle's ring
extern "C" HIPFEAT_RAGGED_API hipfeat_status hipfeat_grad_run_ragged(hipfeat_grad* g, const float* d_wave, int64_t batch, int64_t max_samples, int64_t row_stride,
                                                                   const int64_t* h_lengths, const float* d_grad_out, int64_t grad_out_floats,
                                                                   const float* d_grad_log_energy, float* d_grad_wave, int64_t grad_wave_stride,
                                                                   float* d_workspace, int64_t workspace_floats, void* stream) {
  if (!g) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (batch < 0 || max_samples < 0 || grad_out_floats < 0 || workspace_floats < 0) return fail(HIPFEAT_ERR_INVALID, "negative size");
  if (batch > 0 && !h_lengths) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (batch > 1 && (row_stride < max_samples || grad_wave_stride < max_samples))
    return fail(HIPFEAT_ERR_INVALID, "a row stride is shorter than its row (waveform %lld, gradient %lld, max_samples = %lld)", (long long)row_stride,
                (long long)grad_wave_stride, (long long)max_samples);
  std::vector<int64_t> table;
  int64_t T = 0;  // Tmax
  if (hipfeat_status bad = ragged_table(h_lengths, batch, max_samples, g->N, g->shift, g->snip, table, &T)) return bad;
  if (batch == 0 || max_samples == 0) return HIPFEAT_OK;
  GradPieces pc;
  if (!grad_pieces(batch, T, g->N, 0, &pc) || (T > 0 && batch > INT64_MAX / T / g->width))
    return fail(HIPFEAT_ERR_INVALID, "%lld x %lld frames overflow", (long long)batch, (long long)T);
  const bool frames_mode = g->mode == GRAD_FRAMES;
  if (!d_grad_out && !frames_mode) return fail(HIPFEAT_ERR_INVALID, "NULL device pointer (only a frames handle takes a NULL output cotangent)");
  if (d_grad_out && grad_out_floats < batch * T * g->width)
    return fail(HIPFEAT_ERR_INVALID, "output cotangent of %lld floats, %lld x %lld x %lld needed", (long long)grad_out_floats, (long long)batch, (long long)T,
                (long long)g->width);
  if (!d_wave || !d_grad_wave) return fail(HIPFEAT_ERR_INVALID, "NULL device pointer");
  if (T > 0 && (!d_workspace || workspace_floats < pc.row_floats))
    return fail(HIPFEAT_ERR_INVALID, "workspace of %lld floats, one row of %lld frames needs %lld", (long long)workspace_floats, (long long)T, (long long)pc.row_floats);
  if (reinterpret_cast<uintptr_t>(d_wave) % 4 || reinterpret_cast<uintptr_t>(d_grad_out) % 4 || reinterpret_cast<uintptr_t>(d_grad_log_energy) % 4 ||
      reinterpret_cast<uintptr_t>(d_grad_wave) % 4 || reinterpret_cast<uintptr_t>(d_workspace) % 16)
    return fail(HIPFEAT_ERR_INVALID, "misaligned device pointer (samples, cotangents and gradient: 4 bytes, workspace: 16)");
  const int64_t fpb = 4 * kStftFramesPerWave, bpr = (T + fpb - 1) / fpb, gpr = (max_samples + 3) / 4 + 1;
  if (bpr > INT32_MAX || gpr > (int64_t)INT32_MAX * 128) return fail(HIPFEAT_ERR_UNSUPPORTED, "a row of %lld samples is too long for one launch", (long long)max_samples);
  int64_t rpp = T > 0 ? workspace_floats / pc.row_floats : batch;
  rpp = std::min({rpp, batch, T > 0 ? INT32_MAX / bpr : batch, (int64_t)INT32_MAX * 128 / gpr});
  GradParams p{};
  GradOlaParams o{};
  fill_grad_params(g, pc, max_samples, T, row_stride, grad_wave_stride, d_workspace, bpr, gpr, p, o);
  std::lock_guard<std::mutex> lk(g->mu);
  DeviceGuard guard(g->device);
  hipStream_t st = (hipStream_t)stream;
  StagedSlot& slot = g->ring.take();
  const size_t bytes = table.size() * sizeof(int64_t);
  HIP_TRY(stage(slot, bytes, bytes, st, [&](unsigned char* h) { std::memcpy(h, table.data(), bytes); }));
  set_lds_poison(g->lds);
  for (int64_t r0 = 0; r0 < batch; r0 += rpp) {
    const int64_t rows = std::min(rpp, batch - r0);
    p.wave = d_wave + r0 * row_stride;
    p.gout = d_grad_out ? d_grad_out + r0 * T * g->width : nullptr;
    p.glog_e = (g->energy_rows && d_grad_log_energy) ? d_grad_log_energy + r0 * T : nullptr;
    o.gwave = d_grad_wave + r0 * grad_wave_stride;
    o.rows = rows;
    RaggedArgs a{static_cast<const int64_t*>(slot.d) + 2 * r0, 0.f};
    const int64_t* ola_table = a.table;
    void* pa[] = {&p, &a};
    void* oa[] = {&o, &ola_table};
    if (T > 0) (void)hipLaunchKernel(g->fn_ragged, dim3((unsigned)(rows * bpr)), dim3(256), pa, g->lds, st);
    (void)hipLaunchKernel(reinterpret_cast<const void*>(grad_overlap_add_ragged_kernel), dim3((unsigned)((rows * gpr + 255) / 256)), dim3(256), oa, 0, st);
  }
  return finish_launches(slot, st, hipGetLastError(), "ragged gradient", kWaitedLaunches);
}

// ---- bulk save path: per-batch host work of the offline driver (host_bulk.hpp) -------------------------------------------------
struct hipfeat_archive {
  hipfeat::ArchiveFiles files;
  std::mutex mu;
};

extern "C" HIPFEAT_API hipfeat_status hipfeat_archive_open(const char* const* h_paths, int32_t num_files, int32_t append, hipfeat_archive** out) {
  if (!out) return fail(HIPFEAT_ERR_INVALID, "archive pointer is NULL");
  *out = nullptr;
  if (!h_paths || num_files < 1 || num_files > 64) return fail(HIPFEAT_ERR_INVALID, "an archive has 1 ... 64 files");
  hipfeat_archive* a = new (std::nothrow) hipfeat_archive();
  if (!a) return fail(HIPFEAT_ERR_INVALID, "out of host memory");
  for (int32_t k = 0; k < num_files; ++k) {
    const int fd = h_paths[k] ? ::open(h_paths[k], O_CREAT | O_WRONLY | O_CLOEXEC | (append ? 0 : O_TRUNC), 0644) : -1;
    const off_t end = fd >= 0 ? ::lseek(fd, 0, SEEK_END) : (off_t)-1;
    if (fd < 0 || end < 0) {
      const int e = errno;
      if (fd >= 0) ::close(fd);
      for (int f : a->files.fds) ::close(f);
      delete a;
      return fail(HIPFEAT_ERR_INVALID, "cannot open archive file %d (%s): %s", k, h_paths[k] ? h_paths[k] : "NULL", strerror(e));
    }
    a->files.fds.push_back(fd);
    a->files.size.push_back((int64_t)end);
  }
  if (num_files > 1) a->files.pool = new hipfeat::WorkPool(num_files - 1, "hipfeat-stripe");
  *out = a;
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_archive_append(hipfeat_archive* a, const void* h_matrix, int64_t batch, const int64_t* h_num_frames,
                                                             int32_t cols, int32_t bytes_per_value, int32_t* h_file, int64_t* h_byte_offset) {
  if (!a || !h_num_frames || (batch > 0 && !h_matrix) || batch < 0) return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (cols <= 0 || (bytes_per_value != 2 && bytes_per_value != 4)) return fail(HIPFEAT_ERR_INVALID, "rows are %d values of %d bytes: need cols > 0 and 2- or 4-byte values", cols, bytes_per_value);
  for (int64_t i = 0; i < batch; ++i)
    if (h_num_frames[i] < 0) return fail(HIPFEAT_ERR_INVALID, "cut %lld: %lld frames", (long long)i, (long long)h_num_frames[i]);
  std::lock_guard<std::mutex> lk(a->mu);
  int errfile = 0;
  const int e = a->files.append(static_cast<const char*>(h_matrix), batch, h_num_frames, (int64_t)cols * bytes_per_value, bytes_per_value == 2, h_file,
                                h_byte_offset, &errfile);
  if (e == hipfeat::kErrNotFinite16)
    return fail(HIPFEAT_ERR_INVALID, "the batch holds values that are not finite in binary16 (|x| > 65504, inf or nan): nothing was written");
  if (e) return fail(HIPFEAT_ERR_INVALID, "write to archive file %d failed: %s", errfile, strerror(e));
  return HIPFEAT_OK;
}

extern "C" HIPFEAT_API int64_t hipfeat_archive_size(const hipfeat_archive* a, int32_t file) {
  return (a && file >= 0 && file < (int32_t)a->files.size.size()) ? a->files.size[(size_t)file] : -1;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_archive_close(hipfeat_archive* a) {
  if (!a) return HIPFEAT_OK;
  int bad = 0;
  for (int fd : a->files.fds)
    if (::close(fd) != 0) bad = errno;
  delete a->files.pool;
  delete a;
  return bad ? fail(HIPFEAT_ERR_INVALID, "closing an archive file failed: %s", strerror(bad)) : HIPFEAT_OK;
}

extern "C" HIPFEAT_API hipfeat_status hipfeat_manifest_lines(const char* h_heads, const int64_t* h_head_offsets, const char* h_tails,
                                                             const int64_t* h_tail_offsets, int64_t batch, const int64_t* h_num_frames,
                                                             const int64_t* h_expected_frames, const char* h_mids, const int64_t* h_mid_offsets,
                                                             int32_t num_files, const int32_t* h_file, const int64_t* h_byte_offset, int32_t cols,
                                                             int32_t bytes_per_value, char* h_out, int64_t out_capacity, int64_t* h_out_bytes) {
  if (!h_heads || !h_head_offsets || !h_tails || !h_tail_offsets || !h_num_frames || !h_mids || !h_mid_offsets || !h_byte_offset || !h_out || !h_out_bytes)
    return fail(HIPFEAT_ERR_INVALID, "NULL argument");
  if (batch < 0 || num_files < 1 || cols <= 0 || (bytes_per_value != 2 && bytes_per_value != 4)) return fail(HIPFEAT_ERR_INVALID, "bad batch / file / row arguments");
  hipfeat::BulkError err;
  const int64_t n = hipfeat::manifest_lines(h_heads, h_head_offsets, h_tails, h_tail_offsets, batch, h_num_frames, h_expected_frames, h_mids, h_mid_offsets,
                                            num_files, h_file, h_byte_offset, cols, bytes_per_value, h_out, out_capacity, &err);
  if (n < 0) {
    *h_out_bytes = err.index < 0 ? err.a : 0;
    if (err.index >= 0 && err.what[0] == 'f' && err.what[1] == 'r')
      return fail(HIPFEAT_ERR_INVALID, "cut %lld of the batch: %lld frames extracted, its manifest states %lld (the frame-count contract of validate_features)",
                  (long long)err.index, (long long)err.a, (long long)err.b);
    return fail(HIPFEAT_ERR_INVALID, "%s (cut %lld: %lld vs %lld)", err.what, (long long)err.index, (long long)err.a, (long long)err.b);
  }
  *h_out_bytes = n;
  return HIPFEAT_OK;
}

#include "host_pipeline.hpp"

#ifdef HIPFEAT_PHASE_TIMERS
// experiment builds only: install the per-wave phase-clock buffer ([waves][8] uint64, device memory)
extern "C" HIPFEAT_API int hipfeat_debug_set_phase_buffer(unsigned long long* d_buf) {
  return hipMemcpyToSymbol(HIP_SYMBOL(hipfeat::g_phase_buf), &d_buf, sizeof(d_buf)) == hipSuccess ? 0 : 1;
}
#endif
