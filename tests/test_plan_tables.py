"""CPU: the constant tables a plan uploads (lhotse_amd/csrc/plan_tables.hpp), built by the same pure host code through the C shim
tests/native/plan_tables_capi.cpp.

A  tests/golden/plan_tables.json: kernel name, (byte length, crc32) of every upload of hipfeat_plan_create in upload order and the scalars
   the plan keeps, recorded on an MI355X from the commit BEFORE the tables moved into the header (its upload() patched to log them).
   The builders must reproduce the claiming setup's tables and scalars bit for bit, and the whole kernel name.
B  the layouts stated independently in numpy: window halves, pass / split-step twiddles, padded filterbank tables."""
import ctypes
import json
import os
import re
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from lhotse_amd import constants as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_tables.json")
SPEC, LOGSPEC, FBANK, MFCC, WHISPER, LIBROSA = range(6)
NO_COLUMN = 1 << 20  # kMel4NoColumn


def case(name, kind, sr, N, shift, fft, M=0, ceps=0, env=None, **flags):
    return dict(name=name, kind=kind, sr=sr, N=N, shift=shift, fft=fft, M=M, ceps=ceps, env=env or {}, flags=flags)


B512 = {"HIPFEAT_FFT512_VARIANT": "b"}
B256 = {"HIPFEAT_FFT256_VARIANT": "b"}
NOFIX = {"HIPFEAT_NO_FIXED_SCHEDULE": "1"}
PLAIN = dict(remove_dc_offset=0, preemph_coeff=0.0)
CASES = [
    # fft512c: mode 0 at 10 / 13 / 16 rows, mode 1 (one set of 32 steps), MFCC modes 2 and 3
    case("fft512c_fbank80_r13", FBANK, 16000, 400, 160, 512, 80),
    case("fft512c_fbank80_r10", FBANK, 16000, 320, 160, 512, 80),
    case("fft512c_fbank80_r16", FBANK, 16000, 512, 128, 512, 80),
    case("fft512c_fbank64_short13", FBANK, 16000, 360, 120, 512, 64),
    case("fft512c_fbank40_mode1", FBANK, 16000, 400, 160, 512, 40),
    case("fft512c_fbank23", FBANK, 16000, 400, 160, 512, 23),
    case("fft512c_mfcc40_mode2", MFCC, 16000, 400, 160, 512, 40, 13),
    case("fft512c_mfcc23_mode3", MFCC, 16000, 400, 160, 512, 23, 13),
    case("fft512c_mfcc23_nolifter_r16", MFCC, 16000, 512, 128, 512, 23, 20, cepstral_lifter=0),
    case("fft512b_fbank80_r16_lds", FBANK, 16000, 512, 160, 512, 80),  # fft512c declines: 84 KB of LDS
    # fft512 "b"
    case("fft512b_fbank80", FBANK, 16000, 400, 160, 512, 80, env=B512),
    case("fft512b_fbank80_r10", FBANK, 16000, 320, 160, 512, 80, env=B512),
    case("fft512b_mfcc23", MFCC, 16000, 400, 160, 512, 23, 13, env=B512),
    case("fft512b_mfcc40_r16", MFCC, 16000, 512, 160, 512, 40, 40, env=B512),
    case("fft512b_spectrogram", SPEC, 16000, 400, 160, 512),
    case("fft512b_logspectrogram_mag", LOGSPEC, 16000, 400, 160, 512, use_fft_mag=1),
    # fft256c / fft256 "b"
    case("fft256c_fbank40_r13", FBANK, 8000, 200, 80, 256, 40),
    case("fft256c_fbank80_r13", FBANK, 8000, 200, 80, 256, 80),
    case("fft256c_fbank40_r16", FBANK, 8000, 256, 80, 256, 40),
    case("fft256c_fbank40_short13", FBANK, 8000, 160, 80, 256, 40),
    case("fft256b_fbank40_16k", FBANK, 16000, 160, 80, 256, 40),  # fft256c declines: the filters are too wide for 2 sets x 8 steps
    case("fft256b_fbank40", FBANK, 8000, 200, 80, 256, 40, env=B256),
    case("fft256b_mfcc23", MFCC, 8000, 200, 80, 256, 23, 13),
    case("fft256b_mfcc23_r16", MFCC, 8000, 256, 80, 256, 23, 13),
    case("fft256b_spectrogram", SPEC, 8000, 200, 80, 256),
    # fft1024c: the four fixed-schedule geometries, then generic instances at 20 / 26 / 32 rows
    case("fft1024c_24k_fixed", FBANK, 24000, 600, 240, 1024, 80),
    case("fft1024c_32k_fixed", FBANK, 32000, 800, 320, 1024, 80),
    case("fft1024c_22k_fixed", FBANK, 22050, 551, 220, 1024, 80),
    case("fft1024c_librosa_fixed", LIBROSA, 22050, 1024, 256, 1024, 80, mel="slaney", fmin=80.0, fmax=7600.0, window="hann", use_fft_mag=1, **PLAIN),
    case("fft1024c_24k_r20", FBANK, 24000, 600, 240, 1024, 80, env=NOFIX),
    case("fft1024c_32k_r26_64", FBANK, 32000, 800, 320, 1024, 64),
    case("fft1024c_32k_r32_snip", FBANK, 32000, 1024, 320, 1024, 80, snip_edges=1),
    case("fft1024c_librosa_mag_128", LIBROSA, 22050, 1024, 256, 1024, 128, mel="slaney", window="hann", use_fft_mag=1, **PLAIN),
    # fft2048c: odd / even shift at 18 / 19 / 32 rows, fixed-schedule and generic
    case("fft2048c_44k_fixed", FBANK, 44100, 1102, 441, 2048, 80),
    case("fft2048c_48k_fixed", FBANK, 48000, 1200, 480, 2048, 80),
    case("fft2048c_44k_r18", FBANK, 44100, 1102, 441, 2048, 80, env=NOFIX),
    case("fft2048c_48k_r19_64", FBANK, 48000, 1200, 480, 2048, 64),
    case("fft2048c_44k_r32_odd", FBANK, 44100, 1764, 441, 2048, 80),
    case("fft2048c_librosa_r32_even", LIBROSA, 44100, 2048, 512, 2048, 128, mel="slaney", window="hann", **PLAIN),
    # whisper: 80 / 128 filters on whisper3 and whisper2
    case("whisper3_80", WHISPER, 16000, 400, 160, 400, 80, mel="slaney", window="hann_periodic", **PLAIN),
    case("whisper3_128", WHISPER, 16000, 400, 160, 400, 128, mel="slaney", window="hann_periodic", **PLAIN),
    case("whisper2_80", WHISPER, 16000, 400, 160, 400, 80, mel="slaney", window="hann_periodic", env={"HIPFEAT_WHISPER_VARIANT": "2"}, **PLAIN),
    case("whisper2_128", WHISPER, 16000, 400, 160, 400, 128, mel="slaney", window="hann_periodic", env={"HIPFEAT_WHISPER_VARIANT": "2"}, **PLAIN),
    # wave-per-frame kernel: H = 256 / 512 / 1024
    case("wave_h256_energy", FBANK, 16000, 400, 160, 512, 80, use_energy=1),
    case("wave_h512_mfcc", MFCC, 24000, 600, 240, 1024, 40, 13),
    case("wave_h512_oddshift", FBANK, 22050, 551, 221, 1024, 80),
    case("wave_h1024_mfcc80", MFCC, 44100, 1102, 441, 2048, 80, 40),
    case("wave_h1024_logspec", LOGSPEC, 48000, 1200, 480, 2048),
]


def plan_inputs(c):
    """(config, window, mel, dct, lifter) of hipfeat_plan_create for a case, as lhotse_amd.extractors derives them."""
    f = dict(snip_edges=0, remove_dc_offset=1, use_energy=0, raw_energy=1, use_fft_mag=0, preemph_coeff=0.97, cepstral_lifter=22, mel="kaldi",
             window="povey")
    f.update(c["flags"])
    kind, N, fft, M, ceps = c["kind"], c["N"], c["fft"], c["M"], c["ceps"]
    if kind == LIBROSA:
        window = C.make_stft_window(f["window"], N, fft)
    else:
        window = C.make_window(N, f["window"])
    mel = dct = lifter = None
    if M:
        mel = C.make_slaney_mel(M, fft, c["sr"], f.get("fmin", 0.0), f.get("fmax")) if f["mel"] == "slaney" else C.make_kaldi_mel(M, fft, c["sr"], 20.0, -400.0)
        mel = np.ascontiguousarray(mel, dtype=np.float32)
    if kind == MFCC:
        dct = C.make_dct(ceps, M)
        lifter = C.make_lifter(ceps, f["cepstral_lifter"])
    cfg = dict(kind=kind, frame_length=N, frame_shift=c["shift"], fft_length=fft, num_filters=M, num_ceps=ceps, snip_edges=f["snip_edges"],
               remove_dc_offset=f["remove_dc_offset"], use_energy=f["use_energy"], raw_energy=f["raw_energy"], use_fft_mag=f["use_fft_mag"],
               apply_lifter=int(kind == MFCC and f["cepstral_lifter"] > 0), preemph_coeff=f["preemph_coeff"], energy_floor=float(np.finfo(np.float32).eps),
               mel_floor=C.MEL_FLOOR, log_offset=C.LOG_SPEC_OFFSET, dither=0.0, batch_hop=c["shift"])
    return cfg, window, mel, dct, lifter


# --------------------------------------------------------------------------------------------------------------------------------
# the shim
# --------------------------------------------------------------------------------------------------------------------------------
# The geometry constants the setups in hipfeat.hip pass to the builders, read from where the kernels define them (`constexpr int` in the headers
# next to the device code, which g++ cannot include): a changed constant changes what this test builds.
def kernel_constants():
    env = {}
    for fn in sorted(os.listdir(os.path.join(ROOT, "lhotse_amd", "csrc"))):
        if fn.endswith(".hpp"):
            with open(os.path.join(ROOT, "lhotse_amd", "csrc", fn)) as f:
                for decl in re.findall(r"^constexpr int (k\w+ = [^;]+);", f.read(), flags=re.M):
                    for item in re.split(r",\s*(?=k\w+ = )", decl):
                        name, expr = item.split(" = ")
                        if re.fullmatch(r"[\w\s+*/()-]+", expr):
                            env[name] = eval(expr.replace("/", "//"), {}, env)
    return env


K = kernel_constants()
GEOM = {  # prow_stride, max_sets, max_steps, waves, region, then the family's extras
    "fft512c": [K["kCPRowStride"], K["kCMaxSets"], K["kCMaxSteps"], K["kCWaves"], K["kCRegion"], K["kCDctChunks"], K["kCDctChunksSmall"]],
    "fft256c": [K["kDPRowStride"], K["kDSets"], K["kDSteps"], K["kDWaves"], K["kDRegion"]],
    "fft1024c": [K["kWPRowStride"], K["kWMaxSets"], K["kWMaxSteps"], K["kWWaves"], K["kWRegion"], K["kWSplitSteps"], K["kWWavesFixed"]],
    "fft2048c": [K["kXPRowStride"], K["kXMaxSets"], K["kXMaxSteps"], K["kXMaxWaves"], K["kXRegion"], K["kXSplitSteps"], K["kXWavesFixed"]],
    "whisper3": [K["kW3PRowStride"], K["kW3MaxSets"], K["kW3Steps"], K["kW3Waves"], K["kW3Region"], K["kW3Span"], K["kW3Tail"]],
    # lanes, prow_stride, max_groups0, max_groups1, tile_frames, wave_region, rotated split
    "fft512b": [16, K["kPRowStride"], K["kMaxGroups0"], K["kMaxGroups1"], K["kTileFrames"], K["kBWaveRegion"], 0],
    "fft256b": [8, K["k256PRowStride"], K["kMaxGroups0"], K["kMaxGroups1"], K["k256TileFrames"], K["k256WaveRegion"], 1],
}
WAVE_AUTO_SCALARS = ["lds", "shared_floats", "wtab_off", "ltab_off", "xs_floats", "waves", "mode", "nrows", "sch_nsets", "sch_steps", "w_nsets", "w_steps0",
                     "w_steps1", "w_steps2", "w_steps3", "w_step00", "w_step01", "w_step02", "w_step03", "tws_off", "tw32_off", "fixed", "w12"]
SCALARS = {"tile": ["lds", "xs_floats", "lm_stride", "dct_groups", "nrows"], "whisper2": ["load0", "load1", "load2", "load3"], "wave": ["lds", "dct_in_lds"],
           "band": ["lo", "hi"]}


@pytest.fixture(scope="module")
def lib():
    out = os.path.join(tempfile.mkdtemp(prefix="plantab_"), "libplantab.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "native", "plan_tables_capi.cpp"), "-o", out])
    lib = ctypes.CDLL(out)
    lib.pt_table_bytes.restype = ctypes.c_longlong
    lib.pt_scalar.restype = ctypes.c_longlong
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def build(lib, family, inputs, args):
    """-> (tables as bytes in upload order, scalars by name), or None when the configuration does not fit the family's schedule."""
    cfg, window, mel, dct, lifter = inputs
    in5 = np.array([cfg["frame_length"], cfg["frame_shift"], cfg["fft_length"] // 2 + 1, cfg["num_filters"], cfg["num_ceps"]], dtype=np.int32)
    a = np.array(list(args) + [0] * 16, dtype=np.int32)
    rc = lib.pt_build(family.encode(), _ptr(in5), _ptr(window), _ptr(mel), _ptr(dct), _ptr(lifter if cfg["apply_lifter"] else None), _ptr(a))
    assert rc >= 0, family
    if rc == 0:
        return None
    tables = []
    for i in range(lib.pt_num_tables()):
        buf = ctypes.create_string_buffer(max(1, lib.pt_table_bytes(i)))
        lib.pt_table_copy(i, buf)
        tables.append(buf.raw[: lib.pt_table_bytes(i)])
    names = SCALARS.get(family, WAVE_AUTO_SCALARS)
    assert lib.pt_num_scalars() == len(names)
    return tables, {n: lib.pt_scalar(i) for i, n in enumerate(names)}


def floats(table):
    return np.frombuffer(table, dtype=np.float32)


# --------------------------------------------------------------------------------------------------------------------------------
# A: the same bytes as the commit before
# --------------------------------------------------------------------------------------------------------------------------------
def rows_of(c):
    """Window rows of a case: what the setups in hipfeat.hip derive from the frame length (and, fft 2048, the parity of the shift)."""
    N, fft = c["N"], c["fft"]
    if fft == 2048:
        need, small = (N + 63) // 64, (18 if c["shift"] & 1 else 19)
        return small if need <= small else 32
    need = (N + 15) // 16 if fft == 256 else (N + 31) // 32
    for r in {256: (13, 16), 512: (10, 13, 16), 1024: (20, 26, 32)}[fft]:
        if need <= r:
            return r


def fixed_steps(c, nrows):
    """The schedule of the fixed-schedule instance that has the case's configuration compiled in (setup_fft1024c / setup_fft2048c), or None."""
    f = c["flags"]
    kaldi80 = c["kind"] == FBANK and c["M"] == 80 and not f.get("use_fft_mag") and not f.get("snip_edges")
    if "HIPFEAT_NO_FIXED_SCHEDULE" in c["env"]:
        return None
    if c["fft"] == 1024 and nrows == 32:
        return [16, 16, 8] if f.get("remove_dc_offset", 1) == 0 and f.get("preemph_coeff", 0.97) == 0.0 else None
    if c["fft"] == 1024 and kaldi80:
        return {(600, 240): [24, 16, 8], (800, 320): [24, 16, 8], (551, 220): [24, 24, 8]}.get((c["N"], c["shift"]))
    if c["fft"] == 2048 and kaldi80 and (c["N"], c["shift"]) in ((1102, 441), (1200, 480)):
        return [52, 28, 16]
    return None


def expected_of(lib, c, kernel_name):
    """From the builders: the tables the claiming setup uploads, in upload order; the plan's scalars by their recorded names; the plan's
    whole kernel name, `{cu}` standing for the one part that is read from the device (the occupancy of the instance)."""
    inputs = plan_inputs(c)
    fam = kernel_name.split("_kernel")[0]
    nrows = rows_of(c) if c["fft"] in (256, 512, 1024, 2048) else 0
    fx = fixed_steps(c, nrows)
    fixed_args = [1] + fx if fx else [0, 0, 0, 0]
    if fam in ("fft512b", "fft256"):
        kernel, fam = fam + "_kernel", ("fft512b" if fam == "fft512b" else "fft256b")
        tables, s = build(lib, "tile", inputs, [nrows] + GEOM[fam])
        consts, mel_a, work, mel_a4, dct = tables
        out, what = (1, "mfcc") if c["kind"] == MFCC else ((2, "spectrogram") if c["kind"] in (SPEC, LOGSPEC) else (0, "fbank"))
        up = [consts] + ([mel_a] if fam == "fft512b" else []) + [work, mel_a4] + ([dct] if c["kind"] == MFCC else [])
        return up, dict(lds=s["lds"], xs_floats=s["xs_floats"], const_floats=len(consts) // 4, lm_stride=s["lm_stride"], dct_groups=s["dct_groups"],
                        dct_floats=len(dct) // 4, tiles_per_block=16, block=256, fpb=16 * GEOM[fam][4]), \
            "%s<%d,%d> %s lds=%dB blocks/CU={cu}" % (kernel, s["nrows"], out, what, s["lds"])
    if fam == "wave":
        tables, s = build(lib, "wave", inputs, [c["fft"] // 2])
        return ([tables[0]] if c["M"] else []), dict(lds=s["lds"], wave_blob_floats=len(tables[0]) // 4, wave_dct_in_lds=s["dct_in_lds"], block=256, fpb=32), \
            "wave_kernel<%d> fft=%d lds=%dB blocks/CU={cu}" % (c["fft"] // 128, c["fft"], s["lds"])
    w2 = build(lib, "whisper2", inputs, [])
    if fam == "whisper":  # whisper_kernel2
        loads = "+".join(str(w2[1]["load%d" % i]) for i in range(4))
        return w2[0], dict(lds=0, block=256, fpb=128), "whisper_kernel2 fft400=16x25 mel_chunks=%s blocks/CU={cu}" % loads
    args = {"fft512c": [nrows] + GEOM["fft512c"], "fft256c": [nrows] + GEOM["fft256c"], "fft1024c": [nrows] + GEOM["fft1024c"] + fixed_args,
            "fft2048c": [nrows] + GEOM["fft2048c"] + fixed_args + [c["shift"] & 1, 160 * 1024], "whisper3": [0] + GEOM["whisper3"]}[fam]
    tables, s = build(lib, fam, inputs, args)
    frames, rounds, rounds_max = {"fft512c": (4, 8, 16), "fft256c": (8, 4, 16), "fft1024c": (4, 8, 32), "fft2048c": (2, 8, 64), "whisper3": (4, 8, 16)}[fam]
    want = dict(lds=s["lds"], block=64 * s["waves"], fpb_unit=frames * s["waves"], fpb=frames * s["waves"] * rounds, c_rounds_max=rounds_max,
                c_shared_floats=s["shared_floats"], c_wtab_off=s["wtab_off"], c_ltab_off=s["ltab_off"], c_xs_floats=s["xs_floats"], x_tws_off=s["tws_off"],
                x_tw32_off=s["tw32_off"], w_nsets=s["w_nsets"], w_steps=[s["w_steps%d" % i] for i in range(4)], w_step0=[s["w_step0%d" % i] for i in range(4)],
                x_waves=s["waves"] if fam == "fft2048c" else 0)
    fixed_waves = "%s waves=%d" % (" fixed-schedule" if s["fixed"] else "", s["waves"])
    head = {"fft512c": "fft512c_kernel<%d> %s" % (s["nrows"], "mfcc" if c["kind"] == MFCC else "fbank"), "fft256c": "fft256c_kernel<%d> fbank" % s["nrows"],
            "fft1024c": "fft1024c_kernel<%d> fbank%s" % (s["nrows"], fixed_waves), "fft2048c": "fft2048c_kernel<%d,%d> fbank%s" % (s["nrows"], c["shift"] & 1, fixed_waves),
            "whisper3": "whisper3_kernel<%d> fft400=16x25 fused-norm" % s["w_nsets"]}[fam]
    return (w2[0] if fam == "whisper3" else []) + tables, want, head + " lds=%dB blocks/CU={cu} mel4=%dx%d" % (s["lds"], s["sch_nsets"], s["sch_steps"])


with open(GOLDEN) as _f:
    RECORD = json.load(_f)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_tables_and_scalars_equal_the_recorded_plan(lib, c):
    rec = RECORD[c["name"]]
    tables, scalars, name = expected_of(lib, c, rec["kernel_name"])
    cu = re.search(r" blocks/CU=([1-9]\d*)", rec["kernel_name"])  # at least one workgroup per CU, whatever the device says beyond that
    assert cu and rec["kernel_name"] == name.format(cu=cu.group(1))
    got = [[len(t), zlib.crc32(t)] for t in tables]
    # the uploads of hipfeat_plan_create itself come first: twiddles, window (, filterbank, bands) (, DCT (, lifter))
    cfg, window, mel, dct, lifter = plan_inputs(c)
    fft = c["fft"]
    head = [[8 * (fft // 2 if fft & (fft - 1) == 0 else fft)], window]  # W_fft^k (length only: the generic kernel's table stayed where it was)
    if mel is not None:  # the filterbank and the band of every filter: [first non-zero bin, last non-zero bin + 1), (0, 0) for an empty one
        nz = mel != 0
        lo, hi = nz.argmax(axis=0), mel.shape[0] - nz[::-1].argmax(axis=0)
        head += [mel, np.where(nz.any(axis=0), np.stack([lo, hi]), 0).T.astype(np.int32)]
    if dct is not None:
        head += [dct] + ([lifter] if cfg["apply_lifter"] else [])
    head = [h if isinstance(h, list) else [h.nbytes, zlib.crc32(np.ascontiguousarray(h).tobytes())] for h in head]
    assert len(rec["uploads"]) == len(head) + len(got)
    assert [u[: len(h)] for u, h in zip(rec["uploads"], head)] == head
    assert rec["uploads"][len(head):] == got
    for k, v in scalars.items():
        assert rec["scalars"][k] == v, k


def test_the_record_covers_every_route_and_instance_family():
    names = {c["name"]: RECORD[c["name"]]["kernel_name"] for c in CASES}
    assert set(RECORD) == set(names)

    def has(*parts):
        return any(all(p in n for p in parts) for n in names.values())

    for rows in (10, 13, 16):
        assert has("fft512c_kernel<%d> fbank" % rows)
    modes = set()
    for c in CASES:  # fft512c modes: 0 / 1 by the padded table shape (2 x 16 or 1 x 32 steps), 2 / 3 MFCC with more / at most 24 filters
        if names[c["name"]].startswith("fft512c"):
            modes.add((3 if c["M"] <= 24 else 2) if c["kind"] == MFCC else int(RECORD[c["name"]]["scalars"]["c_shared_floats"] - RECORD[c["name"]]["scalars"]["c_ltab_off"] < 512))
    assert modes == {0, 1, 2, 3}
    for what in ("fbank", "mfcc", "spectrogram"):
        assert has("fft512b_kernel<", what)
    assert has("fft256c_kernel<13>") and has("fft256c_kernel<16>") and has("fft256_kernel<", "mfcc")
    for rows in (20, 26, 32):
        assert has("fft1024c_kernel<%d>" % rows)
    assert sum("fft1024c" in n and "fixed-schedule" in n for n in names.values()) == 4
    for inst in ("<18,1>", "<32,1>", "<19,0>", "<32,0>"):
        assert has("fft2048c_kernel" + inst)
    for k in ("whisper3_kernel<2>", "whisper3_kernel<3>", "whisper_kernel2"):
        assert has(k)
    assert sum(n.startswith("whisper_kernel2") for n in names.values()) == 2
    for h in (4, 8, 16):
        assert has("wave_kernel<%d>" % h)


# --------------------------------------------------------------------------------------------------------------------------------
# B: the layouts, stated independently
# --------------------------------------------------------------------------------------------------------------------------------
def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def W(k, n):
    """exp(-2 pi i k / n) rounded to float32, as (re, im)."""
    a = -2.0 * np.pi * np.asarray(k, dtype=np.float64) / n
    return np.stack([np.cos(a), np.sin(a)], axis=-1).astype(np.float32)


def minus_i(w):
    return np.stack([w[..., 1], -w[..., 0]], axis=-1)


def image_of(lib, name):
    c = by_name(name)
    fam = name.split("_")[0]
    nrows = rows_of(c)
    extra = {"fft1024c": [0, 0, 0, 0], "fft2048c": [0, 0, 0, 0, c["shift"] & 1, 160 * 1024]}.get(fam, [])
    if fam in ("fft512b", "fft256b"):
        tables, s = build(lib, "tile", plan_inputs(c), [nrows] + GEOM[fam])
    else:
        tables, s = build(lib, fam, plan_inputs(c), [nrows] + GEOM[fam] + extra)
    return c, nrows, floats(tables[0]), s, tables


@pytest.mark.parametrize("name,lanes", [("fft512c_fbank80_r13", 16), ("fft512b_fbank80_r10", 16), ("fft256c_fbank40_short13", 8), ("fft256b_mfcc23_r16", 8),
                                        ("fft1024c_24k_fixed", 16), ("fft2048c_44k_fixed", 32)])
def test_window_halves(lib, name, lanes):
    c, nrows, img, _, _ = image_of(lib, name)
    w = plan_inputs(c)[1]
    got = img[: nrows * lanes * 2].reshape(nrows, lanes, 2)
    for n1 in range(nrows):
        for q in range(lanes):
            for e in range(2):
                i = 2 * lanes * n1 + 2 * q + e  # row n1 holds 2 * lanes samples, lane q an (even, odd) pair of them
                assert got[n1, q, e] == (np.float32(0.5) * w[i] if i < c["N"] else 0.0)
    assert nrows * lanes * 2 >= c["N"] and np.count_nonzero(got.reshape(-1)[c["N"]:]) == 0


@pytest.mark.parametrize("name,lanes,rows,order", [("fft512c_fbank80_r13", 16, 16, 256), ("fft512b_fbank80", 16, 16, 256), ("fft256c_fbank40_r13", 8, 16, 128),
                                                   ("fft256b_mfcc23", 8, 16, 128), ("fft1024c_32k_fixed", 16, 32, 512)])
def test_pass_twiddles(lib, name, lanes, rows, order):
    _, nrows, img, _, _ = image_of(lib, name)
    got = img[nrows * lanes * 2:][: rows * lanes * 2].reshape(rows, lanes, 2)
    k1, q = np.meshgrid(np.arange(rows), np.arange(lanes), indexing="ij")
    assert np.array_equal(got, W(q * k1, order))


def test_fft2048c_pass_twiddles_and_pass2_butterflies(lib):
    _, nrows, img, s, tables = image_of(lib, "fft2048c_48k_fixed")
    k1, q = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    assert np.array_equal(floats(tables[1]).reshape(32, 32, 2), W(q * k1, 1024))
    tw32 = img[s["tw32_off"]:][:64].reshape(2, 16, 2)
    assert np.array_equal(tw32[0], W(np.zeros(16), 32)) and np.array_equal(tw32[1], W(np.arange(16), 32))
    assert s["tws_off"] == nrows * 64 and s["tw32_off"] == s["tws_off"] + 17 * 64 and s["wtab_off"] == s["tw32_off"] + 64


@pytest.mark.parametrize("name,lanes,passf,order,rotated", [("fft512c_fbank80_r16", 16, 512, 512, False), ("fft512b_mfcc23", 16, 512, 512, False),
                                                            ("fft256c_fbank40_r16", 8, 256, 256, False), ("fft256b_fbank40", 8, 256, 256, True)])
def test_split_twiddles_plain_rule(lib, name, lanes, passf, order, rotated):
    _, nrows, img, _, _ = image_of(lib, name)
    got = img[nrows * lanes * 2 + passf:][: 8 * lanes * 2 * (2 if rotated else 1)].reshape(-1, 8, lanes, 2)
    j, q = np.meshgrid(np.arange(8), np.arange(lanes), indexing="ij")
    w = minus_i(W(q + lanes * j, order))  # lane q of step j: bin q + lanes j
    assert np.array_equal(got[0], w)
    if rotated:  # (-w.y, w.x) = i w
        assert np.array_equal(got[1], np.stack([-w[..., 1], w[..., 0]], axis=-1))


@pytest.mark.parametrize("name,lanes,order", [("fft1024c_24k_r20", 16, 1024), ("fft2048c_44k_r32_odd", 32, 2048)])
def test_split_twiddles_where_lane_0_takes_extra_bins(lib, name, lanes, order):
    """Step s < 16 covers the bins [2 lanes s, 2 lanes (s + 1)): lane q >= 1 starts at q + 2 lanes s (fft2048c: lanes above 16 at the mirrored
    bin 64 - q + 64 s) and idles in step 16; lane 0 takes the multiples of 2 lanes up to step 8, then the odd multiples of `lanes`."""
    _, nrows, img, s, _ = image_of(lib, name)
    at = s["tws_off"] if lanes == 32 else nrows * 32 + 32 * 16 * 2
    got = img[at:][: 17 * lanes * 2].reshape(17, lanes, 2)
    k = np.zeros((17, lanes), dtype=np.int64)
    for st in range(16):
        for q in range(1, lanes):
            k[st, q] = (q if (lanes == 16 or q <= 16) else 64 - q) + 2 * lanes * st
    k[:9, 0] = 2 * lanes * np.arange(9)
    k[9:, 0] = lanes + 2 * lanes * np.arange(8)
    assert np.array_equal(got, minus_i(W(k, order)))
    assert sorted(set(k[:, 0])) == sorted(set(2 * lanes * np.arange(9)) | set(lanes + 2 * lanes * np.arange(8)))


@pytest.mark.parametrize("name,tsets,tsteps", [("fft512c_fbank80_r13", 2, 16), ("fft512c_mfcc23_mode3", 1, 32), ("fft256c_fbank40_r13", 2, 8), ("whisper3_80", 2, 16)])
def test_padded_filterbank_tables(lib, name, tsets, tsteps):
    """The kernel runs tsets x tsteps steps whatever the schedule: steps beyond a set's own carry zero weights, sets beyond the
    schedule's zero weights and no output column."""
    c = by_name(name)
    fam = name.split("_")[0]
    tables, s = build(lib, fam, plan_inputs(c), [rows_of(c) if fam != "whisper3" else 0] + GEOM[fam])
    img = floats(tables[-1] if fam != "fft512c" else tables[0])
    assert s["ltab_off"] - s["wtab_off"] == tsets * tsteps * 64 and s["shared_floats"] == len(img) and len(img) % 64 == 0
    assert s["ltab_off"] + tsets * 256 <= len(img) < s["ltab_off"] + tsets * 256 + 64
    wtab = img[s["wtab_off"]: s["ltab_off"]].reshape(tsets, tsteps // 4, 64, 4)
    ltab = img[s["ltab_off"]:][: tsets * 256].reshape(tsets, 64, 4)
    cols = ltab[:, :, 1].view(np.int32)
    assert sorted(cols[cols != NO_COLUMN]) == list(range(c["M"]))  # every filter leaves through exactly one lane
    assert s["sch_nsets"] <= tsets and s["sch_steps"] <= tsets * tsteps
    # the schedule as the shim of mel4_schedule.hpp builds it: the same weights, set by set, zeros behind
    mel = plan_inputs(c)[2]
    used = np.count_nonzero(wtab.reshape(tsets, -1), axis=1)
    for s2 in range(s["sch_nsets"], tsets):
        assert used[s2] == 0 and (cols[s2] == NO_COLUMN).all() and not ltab[s2][:, [0, 2, 3]].any()
    assert np.isclose(wtab.sum(dtype=np.float64), mel.sum(dtype=np.float64), rtol=1e-6)  # every weight is there exactly once


def test_band_of_filter_columns(lib):
    mel = np.zeros((9, 5), dtype=np.float32)
    mel[2:5, 0] = 1.0
    mel[7, 2] = 0.5
    inputs = (dict(frame_length=16, frame_shift=8, fft_length=16, num_filters=5, num_ceps=0, apply_lifter=0), None, mel, None, None)
    band = lambda j0, j1: tuple(build(lib, "band", inputs, [j0, j1])[1].values())
    assert band(0, 1) == (2, 5) and band(1, 2) == (0, 0) and band(2, 3) == (7, 8) and band(0, 5) == (2, 8) and band(3, 16) == (0, 0)
