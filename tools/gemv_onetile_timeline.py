#!/usr/bin/env python3
"""In-kernel timeline of the one-row int4g32 GEMV (build: make -C chatglm_q_amd/csrc timeline).

Every wave of the 16-bit GEMV stamps the 100 MHz s_memrealtime clock at seven stations - entry, staging barrier passed, last weight
word landed, dots done, reductions done, K-slice barrier passed, store issued - and lane 0 writes them into the wave's slot (plain
stores).  The probed launch runs behind 16 launches on other weight sets and an in-stream reset, like bench.py's kernel_span leg.
Printed: the medians over the repetitions of each interval, for the wave that finishes last on the whole chip and for the median over
the CUs of each CU's last-finishing wave (CU = the XCC_ID / SE_ID / SH_ID / CU_ID fields of the wave's hardware id).

The geometry switches are read once per process, so each configuration runs in a child process:
  tile-loop  QLINEAR_DISPATCH=noonetile (the kernel before the one-tile path)
  cw4        one-tile path, 4 columns per wave        cw2   one-tile path, 2 columns per wave (the default dispatch: lean entry)
  cw2-64bit  cw2 behind the entry with 64-bit addresses       cw2-ticket  cw2 with the arrival-ticket quad combine (station 5: ticket returned)
  kc1, kc2   K-complete geometry, 1 / 2 whole columns per wave: no combine across waves, so station 5 does not exist - printed as such,
             and "combined -> stored" is then reduced -> stored
    python tools/gemv_onetile_timeline.py [--configs tile-loop,cw4,cw2] [--K 4096 --N 4096] [--reps 48]
"""
import argparse
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "chatglm_q_amd", "csrc", "libqlinear_hip_timeline.so")
STATIONS = ["entry", "staged", "landed", "dots", "reduced", "combined", "stored"]
# every configuration pins QLINEAR_ONETILE_KC: the library's own default is the geometry that ships
CONFIGS = {"tile-loop": {"QLINEAR_DISPATCH": "noonetile"}, "cw4": {"QLINEAR_ONETILE_CW": "4", "QLINEAR_ONETILE_KC": "0"},
           "cw2": {"QLINEAR_ONETILE_CW": "2", "QLINEAR_ONETILE_KC": "0"},
           "cw2-64bit": {"QLINEAR_ONETILE_CW": "2", "QLINEAR_ONETILE_LEAN": "0", "QLINEAR_ONETILE_KC": "0"},
           "cw2-ticket": {"QLINEAR_ONETILE_CW": "2", "QLINEAR_ONETILE_TICKET": "1", "QLINEAR_ONETILE_KC": "0"},
           "kc1": {"QLINEAR_ONETILE_CW": "2", "QLINEAR_ONETILE_KC": "1"}, "kc2": {"QLINEAR_ONETILE_CW": "2", "QLINEAR_ONETILE_KC": "2"}}
KC_OF = {"kc1": 1, "kc2": 2}                # which configurations must be served by the K-complete kernel (checked by its launch counter)


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def child(args):
    import numpy as np
    import torch
    from chatglm_q_amd import _lib
    from chatglm_q_amd.int4 import hip_ops as h4

    lib = ctypes.CDLL(LIB)
    res, argtypes = _lib.EXPORTS["qlinear_w4g32_fwd_packed"]
    lib.qlinear_w4g32_fwd_packed.restype, lib.qlinear_w4g32_fwd_packed.argtypes = res, argtypes
    lib.qlinear_timeline_reset_async.argtypes = [ctypes.c_void_p]
    lib.qlinear_timeline_read.argtypes = [ctypes.c_void_p]
    lib.qlinear_w4g32_onetile_kc_launches.restype = ctypes.c_uint64
    K, N, dev = args.K, args.N, torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1234)
    packed = []
    for _ in range(args.sets):
        qw = torch.randint(0, 256, (K // 2, N), dtype=torch.uint8, device=dev, generator=g)
        sc = (torch.rand((K // 32, N), device=dev, generator=g) * 0.02 + 0.002).half()
        packed.append(h4.repack_w4g32(qw, sc))
    x = torch.randn(1, K, device=dev, dtype=torch.float16, generator=g)
    out = torch.empty(1, N, device=dev, dtype=torch.float16)
    st = torch.cuda.current_stream(dev).cuda_stream

    def launch(i):
        return lib.qlinear_w4g32_fwd_packed(x.data_ptr(), packed[i % len(packed)].data_ptr(), None, out.data_ptr(), 1, N, K, 32, K, N, 1, 0,
                                            None, 0, st)

    tick_ns = 1e6 / lib.qlinear_timeline_clock_khz()
    slots = lib.qlinear_timeline_slots()
    host = np.zeros((slots, 8), dtype=np.uint64)
    chip, per_cu, spans, waves = [], [], [], 0
    kc0 = lib.qlinear_w4g32_onetile_kc_launches()
    for rep in range(args.reps + 4):
        for w in range(16):
            assert launch(rep * 17 + w) == 0
        assert lib.qlinear_timeline_reset_async(st) == 0 and launch(rep * 17 + 16) == 0
        torch.cuda.synchronize()
        assert lib.qlinear_timeline_read(host.ctypes.data) == 0
        if rep < 4:
            continue
        live = host[host[:, 6] != 0]
        waves = len(live)
        t = live[:, :7].astype(np.int64)
        assert waves and (np.diff(t, axis=1) >= 0).all(), "stations out of order"
        hw = live[:, 7]
        cu = ((hw >> np.uint64(8)) & np.uint64(0xFF)) | ((hw >> np.uint64(32)) << np.uint64(8))   # CU_ID, SH_ID, SE_ID | XCC_ID
        t0 = t[:, 0].min()
        row = lambda r: np.concatenate(([r[0] - t0], np.diff(r), [r[6] - t0]))   # entry skew, six intervals, end since first entry
        chip.append(row(t[t[:, 6].argmax()]))
        lasts = np.array([row(t[cu == c][t[cu == c][:, 6].argmax()]) for c in np.unique(cu)])
        per_cu.append(np.median(lasts, axis=0))
        spans.append(t[:, 6].max() - t0)
        n_cu = len(np.unique(cu))
    kc_launches, launches = lib.qlinear_w4g32_onetile_kc_launches() - kc0, 17 * (args.reps + 4)
    assert kc_launches in (0, launches), (kc_launches, launches)
    no_combine = kc_launches > 0               # the K-complete kernel ran: a wave keeps its columns, station 5 does not exist
    assert no_combine == (args.child in KC_OF), f"{args.child}: the K-complete kernel {'ran' if no_combine else 'did not run'}"
    names = ["entry after first wave's"] + [f"{a} -> {b}" for a, b in zip(STATIONS, STATIONS[1:])] + ["stored after first wave's entry"]
    chip, per_cu = np.median(np.array(chip), axis=0) * tick_ns, np.median(np.array(per_cu), axis=0) * tick_ns
    print(f"## {args.child}: 1x{K}->{N} fp16, {waves} waves on {n_cu} CUs, {args.reps} probed launches, clock tick {tick_ns:.0f} ns")
    print(f"{'interval (ns, median)':34s} {'last wave of the chip':>22s} {'last wave of a CU (median CU)':>30s}")
    for i, nm in enumerate(names):
        if no_combine and nm == "reduced -> combined":
            print(f"{nm:34s} {'none':>22s} {'none':>30s}   (no combine across waves: the next row is reduced -> stored)")
            continue
        print(f"{nm:34s} {chip[i]:22.0f} {per_cu[i]:30.0f}")
    print(f"{'first entry -> last store (span)':34s} {median(spans) * tick_ns:22.0f}")
    sys.stdout.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="tile-loop,cw4,cw2")
    ap.add_argument("--K", type=int, default=4096)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--sets", type=int, default=72)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if not os.path.exists(LIB):
        raise SystemExit("build the timeline library first: make -C chatglm_q_amd/csrc timeline")
    if args.child:
        return child(args)
    for name in args.configs.split(","):
        env = dict(os.environ, **CONFIGS[name])
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--K", str(args.K), "--N", str(args.N),
                             "--reps", str(args.reps), "--sets", str(args.sets)], env=env, timeout=300).returncode
        if rc != 0:                       # nothing more on the GPU after a failed configuration
            raise SystemExit(f"{name}: exit status {rc}")


if __name__ == "__main__":
    main()
