#!/usr/bin/env python3
"""Kernel-level micro-benchmarks on one MI355X (development tool, not the contract bench).

    python tools/kbench.py mfma | gemm | panel3 | panelx | lu | trsvt | getrs_t | potrf | potri | posx | gecon | gerfs | equil | qr | svd | eig [--n N] [--nb NB]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from linalg_solver_amd import _native as N  # noqa: E402
from linalg_solver_amd import gen  # noqa: E402
from linalg_solver_amd.device import DeviceSolver  # noqa: E402


def timeit(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return min(ts), sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+")
    ap.add_argument("--f32", action="store_true", help="lu: factor in fp32")
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--nb", type=int, default=128)
    args = ap.parse_args()
    dev = DeviceSolver()
    if "qr" in args.what:
        # Householder QR: geqrf beside getrf of the same square matrix, geqrf and gels on tall shapes, and the shares of
        # the panel steps, the T factor (with V and V^T V) and the block applies from the profile buckets
        def shares(fn):
            dev.h.prof_enable(True)
            dev.h.prof_reset()
            fn()
            pr = dev.h.prof_read()
            dev.h.prof_enable(False)
            return "  ".join(f"{k} {pr[k]['ms']:.3f} ms / {pr[k]['launches']}" for k in ("panel", "trsm", "gemm", "other"))

        for dt in ((torch.float32,) if args.f32 else (torch.float64, torch.float32)):
            for n in (4096, 8192):
                A0 = torch.empty(n, n, dtype=dt, device="cuda")
                dev.fill_(A0, gen.U11, 5)
                A = A0.clone()
                tau = torch.zeros(n, dtype=dt, device="cuda")
                ipiv = torch.zeros(n, dtype=torch.int32, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")

                def qrf():
                    A.copy_(A0)
                    dev.geqrf_(A, tau)

                def luf():
                    A.copy_(A0)
                    dev.getrf_(A, ipiv, info)
                tcopy, _ = timeit(lambda: A.copy_(A0), reps=3, warm=1)
                tq, _ = timeit(qrf, reps=3, warm=1)
                tl, _ = timeit(luf, reps=3, warm=1)
                tq, tl = tq - tcopy, tl - tcopy
                print(f"qr {str(dt)[6:]} n={n}: geqrf {tq:.3f} ms ({4 / 3 * n ** 3 / tq / 1e9:.1f} TFLOP/s)  getrf {tl:.3f} ms  "
                      f"| QR/LU {tq / tl:.2f}\n    geqrf shares: {shares(qrf)}", flush=True)
            for m, n in ((16384, 1024), (65536, 256)):
                nrhs = 16
                A0 = torch.empty(m, n, dtype=dt, device="cuda")
                dev.fill_(A0, gen.U11, 6)
                B0 = torch.empty(m, nrhs, dtype=dt, device="cuda")
                dev.fill_(B0, gen.U11, 7)
                A, B = A0.clone(), B0.clone()
                tau = torch.zeros(n, dtype=dt, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")

                def qrf():
                    A.copy_(A0)
                    dev.geqrf_(A, tau)

                def ls():
                    A.copy_(A0)
                    B.copy_(B0)
                    dev.gels_(A, B, tau, info)
                tcopy, _ = timeit(lambda: A.copy_(A0), reps=3, warm=1)
                tq, _ = timeit(qrf, reps=3, warm=1)
                tg, _ = timeit(ls, reps=3, warm=1)
                fl = 2.0 * m * n * n - 2.0 / 3 * n ** 3
                print(f"qr {str(dt)[6:]} {m} x {n}: geqrf {tq - tcopy:.3f} ms ({fl / (tq - tcopy) / 1e9:.1f} TFLOP/s)  gels nrhs={nrhs} "
                      f"{tg - tcopy:.3f} ms\n    geqrf shares: {shares(qrf)}", flush=True)
    if "eig" in args.what:
        # symmetric eigensolver by two-sided Jacobi: syevj with and without vectors beside gesvdj of the same symmetric
        # matrix and torch.linalg.eigh / eigvalsh, in one process; medians of 3 after a warm-up, the restoring copy
        # timed alone and subtracted; sweeps and rotations of the call, rounds (two launches each)
        for dt in ((torch.float32,) if args.f32 else (torch.float64, torch.float32)):
            for n in (512, 1024, 2048):
                G = torch.empty(n, n, dtype=dt, device="cuda")
                dev.fill_(G, gen.U11, 5)
                A0 = ((G + G.T) / 2).contiguous()
                A = A0.clone()
                out = {}

                def ev(v):
                    A.copy_(A0)
                    out[v] = dev.syevj_(A, compute_v=v)[2]

                def sv(uv):
                    A.copy_(A0)
                    dev.gesvdj_(A, compute_uv=uv)
                _, tcopy = timeit(lambda: A.copy_(A0), reps=3, warm=1)
                _, t1 = timeit(lambda: ev(True), reps=3, warm=1)
                sweeps, rot = dev.h.get_option("syevj_sweeps"), dev.h.get_option("syevj_rotations")
                _, t0 = timeit(lambda: ev(False), reps=3, warm=1)
                _, s1 = timeit(lambda: sv(True), reps=3, warm=1)
                _, s0 = timeit(lambda: sv(False), reps=3, warm=1)
                ssweeps = dev.h.get_option("gesvdj_sweeps")
                rounds = (n + (n & 1) - 1) * sweeps
                try:
                    _, tt1 = timeit(lambda: torch.linalg.eigh(A0, UPLO="U"), reps=3, warm=1)
                    _, tt0 = timeit(lambda: torch.linalg.eigvalsh(A0, UPLO="U"), reps=3, warm=1)
                    ref = f"torch.linalg.eigh {tt1:.1f} ms, eigvalsh {tt0:.1f} ms"
                except Exception as e:   # not offered for this type / device
                    ref = f"torch.linalg.eigh not available ({type(e).__name__})"
                print(f"eig {str(dt)[6:]} {n} x {n}: syevj vectors {t1 - tcopy:.1f} ms, values only {t0 - tcopy:.1f} ms "
                      f"(info {out[True]}/{out[False]}, {sweeps} sweeps, {rot} rotations, {rounds} rounds, "
                      f"{(t0 - tcopy) * 1e3 / max(rounds, 1):.1f} us per round without vectors, "
                      f"{(t1 - tcopy) * 1e3 / max(rounds, 1):.1f} us with)  gesvdj vectors {s1 - tcopy:.1f} ms, values only "
                      f"{s0 - tcopy:.1f} ms ({ssweeps} sweeps)  | {ref}", flush=True)
    if "svd" in args.what:
        # Jacobi SVD: gesvdj with and without vectors beside geqrf of the same matrix and, where torch offers it on the
        # device, torch.linalg.svd / svdvals; sweeps and rotations of the call, launches of the round kernel
        for dt in ((torch.float32,) if args.f32 else (torch.float64, torch.float32)):
            for m, n in ((512, 512), (1024, 1024), (2048, 2048), (16384, 256)):
                A0 = torch.empty(m, n, dtype=dt, device="cuda")
                dev.fill_(A0, gen.U11, 5)
                A = A0.clone()
                tau = torch.zeros(min(m, n), dtype=dt, device="cuda")
                out = {}

                def qrf():
                    A.copy_(A0)
                    dev.geqrf_(A, tau)

                def sv(uv):
                    A.copy_(A0)
                    out[uv] = dev.gesvdj_(A, compute_uv=uv)[3]
                tcopy, _ = timeit(lambda: A.copy_(A0), reps=2, warm=1)
                tq, _ = timeit(qrf, reps=2, warm=1)
                t1, _ = timeit(lambda: sv(True), reps=2, warm=1)
                sweeps, rot = dev.h.get_option("gesvdj_sweeps"), dev.h.get_option("gesvdj_rotations")
                t0, _ = timeit(lambda: sv(False), reps=2, warm=1)
                p = min(m, n)
                launches = (p + (p & 1) - 1) * sweeps
                try:
                    tt1, _ = timeit(lambda: torch.linalg.svd(A0, full_matrices=False), reps=2, warm=1)
                    tt0, _ = timeit(lambda: torch.linalg.svdvals(A0), reps=2, warm=1)
                    ref = f"torch.linalg.svd {tt1:.1f} ms, svdvals {tt0:.1f} ms"
                except Exception as e:   # not offered for this type / device
                    ref = f"torch.linalg.svd not available ({type(e).__name__})"
                print(f"svd {str(dt)[6:]} {m} x {n}: gesvdj vectors {t1 - tcopy:.1f} ms, values only {t0 - tcopy:.1f} ms "
                      f"(info {out[True]}/{out[False]}, {sweeps} sweeps, {rot} rotations, {launches} round launches, "
                      f"{(t0 - tcopy) * 1e3 / max(launches, 1):.1f} us per round without vectors)  geqrf {tq - tcopy:.1f} ms  | {ref}",
                      flush=True)
    if "mfma" in args.what:
        for bpc in (1, 2):
            t64, mhz = dev.h.mfma_peak(False, 200000, bpc)
            t32, _ = dev.h.mfma_peak(True, 200000, bpc)
            cyc = 2048.0 * 4 * 256 * bpc * 0 + (mhz * 1e6) / (t64 * 1e12 / (2048.0 * 1024 * (bpc if bpc < 2 else 1) )) if mhz else 0
            print(f"mfma f64 ({bpc} WG/CU = {bpc} wave/SIMD): {t64:.1f} TFLOP/s at {mhz:.0f} MHz in-kernel clock "
                  f"-> {t64 * 1e12 / 1024 / (mhz * 1e6) if mhz else 0:.1f} flop/clk/SIMD "
                  f"(v_mfma_f64_16x16x4 = 2048 flop);   f32: {t32:.1f} TFLOP/s", flush=True)
    if "gemm" in args.what:
        for dt, gw in ((torch.float64, 4), (torch.float64, 8), (torch.float32, 4), (torch.float32, 8)):
            dev.h.set_option("gemm_waves", gw)
            for m, k in ((8064, 128), (4096, 128), (2048, 128), (8064, 256), (4096, 256)):
                A = torch.randn(m, k, dtype=dt, device="cuda")
                B = torch.randn(k, m, dtype=dt, device="cuda")
                Cm = torch.randn(m, m, dtype=dt, device="cuda")
                tmin, tmed = timeit(lambda: dev.gemm_sub_(Cm, A, B))
                fl = 2.0 * m * m * k
                by = 2.0 * Cm.element_size() * m * m
                print(f"gemm_sub {str(dt)[6:]} waves={gw} m=n={m} k={k}: {tmin:.3f} ms  {fl / tmin / 1e9:.1f} TFLOP/s  "
                      f"C traffic {by / tmin / 1e6:.0f} GB/s", flush=True)
    if "gemmq" in args.what:
        # the work-queue form of the update alone: all XCDs / XCD 0 left out, against the plain grid
        dt = torch.float64
        dev.h.set_option("gemm_waves", 0)
        for m, k in ((8064, 128), (6016, 128), (4096, 128), (2048, 128)):
            A = torch.randn(m, k, dtype=dt, device="cuda")
            B = torch.randn(k, m, dtype=dt, device="cuda")
            Cm = torch.randn(m, m, dtype=dt, device="cuda")
            for q in (0, 1, 2):
                dev.h.set_option("gemm_queue_test", q)
                tmin, tmed = timeit(lambda: dev.gemm_sub_(Cm, A, B), reps=7, warm=2)
                fl = 2.0 * m * m * k
                print(f"gemm_sub f64 m=n={m} k={k} queue={q}: min {tmin * 1e3:.1f} us  med {tmed * 1e3:.1f} us  {fl / tmin / 1e9:.1f} TFLOP/s", flush=True)
            dev.h.set_option("gemm_queue_test", 0)
    if "panel3tall" in args.what:
        # the device-scope panel on panels taller than one XCD holds (hybrid driver's first phase, multi-GPU): slice
        # heights (threads per workgroup x rows per thread tile)
        dev.h.set_option("panel", 3)
        for m in (16384, 12288, 9216):
            for nt, rt in ((0, 4), (256, 4), (512, 4), (512, 8), (256, 2), (512, 2)):
                try:
                    dev.h.set_option("panel_nt", nt)
                    dev.h.set_option("panel_rt", rt)
                except Exception as e:
                    print(f"panel3 m={m} nt={nt} rt={rt}: option refused ({e})", flush=True)
                    continue
                P0 = torch.empty(m, args.nb, dtype=torch.float64, device="cuda")
                dev.fill_(P0, gen.U11, 3)
                ipiv = torch.zeros(args.nb, dtype=torch.int32, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")
                P = P0.clone()

                def run():
                    P.copy_(P0)
                    dev.panel_(P, 0, ipiv, info)
                try:
                    tmin, tmed = timeit(run, reps=5, warm=2)
                    tcopy, _ = timeit(lambda: P.copy_(P0), reps=5, warm=2)
                    t = tmin - tcopy
                    print(f"panel3 m={m} nt={nt} rt={rt}: {t * 1e3:.1f} us  ({t * 1e3 / args.nb:.2f} us/col) info={int(info.item())}", flush=True)
                except Exception as e:
                    print(f"panel3 m={m} nt={nt} rt={rt}: failed ({e})", flush=True)
        dev.h.set_option("panel_nt", 0); dev.h.set_option("panel_rt", 4); dev.h.set_option("panel", 4)
    if "panel3" in args.what:
        import numpy as np
        # pipelined panel (mode 3): bitwise check against mode 4, timing, then the stamped build
        dev.h.set_option("panel_rt", 4)
        for m in (args.n, args.n // 2, 1024, 384, 128, 100):
            for nbw in (args.nb, 100):
                P0 = torch.empty(m, nbw, dtype=torch.float64, device="cuda")
                dev.fill_(P0, gen.U11, 3)
                outs = []
                for mode, nt in ((4, 0), (3, 0), (3, 512)):
                    dev.h.set_option("panel", mode)
                    dev.h.set_option("panel_nt", nt)
                    P = P0.clone()
                    ipiv = torch.zeros(nbw, dtype=torch.int32, device="cuda")
                    info = torch.zeros(1, dtype=torch.int32, device="cuda")
                    dev.panel_(P, 0, ipiv, info)
                    torch.cuda.synchronize()
                    outs.append((P, ipiv.clone(), int(info.item())))
                for k in (1, 2):
                    same = torch.equal(outs[0][0], outs[k][0]) and torch.equal(outs[0][1], outs[k][1]) \
                        and outs[0][2] == outs[k][2]
                    print(f"panel3 check m={m} jb={nbw} variant={k}: {'bit-identical' if same else 'MISMATCH'} "
                          f"info={outs[k][2]}", flush=True)
        for mode, nt in ((4, 0), (3, 512), (3, 256)):
            dev.h.set_option("panel", mode)
            dev.h.set_option("panel_nt", nt)
            for m in (args.n, args.n // 2, args.n // 8, 256):
                P0 = torch.empty(m, args.nb, dtype=torch.float64, device="cuda")
                dev.fill_(P0, gen.U11, 3)
                ipiv = torch.zeros(args.nb, dtype=torch.int32, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")
                P = P0.clone()

                def run():
                    P.copy_(P0)
                    dev.panel_(P, 0, ipiv, info)
                tmin, tmed = timeit(run, reps=5, warm=1)
                tcopy, _ = timeit(lambda: P.copy_(P0), reps=5, warm=1)
                t = tmin - tcopy
                print(f"panel mode={mode} nt={nt} m={m} nb={args.nb}: {t * 1e3:.1f} us  ({t * 1e3 / args.nb:.2f} us/col)",
                      flush=True)
        names = ["O1:poll headers+winner", "O2:row granules", "O3:multipliers+block", "next cand+header",
                 "barrier", "bulk+publish", "block boundary", "-"]
        dev.h.set_option("panel", 3)
        dev.h.set_option("panel_debug", 1)
        for nt, m in ((512, args.n), (256, args.n), (512, 1024), (512, 128)):
            dev.h.set_option("panel_nt", nt)
            P = torch.empty(m, args.nb, dtype=torch.float64, device="cuda")
            ipiv = torch.zeros(args.nb, dtype=torch.int32, device="cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")
            for rep in range(2):
                dev.fill_(P, gen.U11, 3)
                dev.panel_(P, 0, ipiv, info)
            torch.cuda.synchronize()
            rows = nt // 16 * 4
            G = (m + rows - 1) // rows
            need = 256 + 2 * G * 512 + 2 * G * 128 * 16
            off = (need + 255) & ~255
            raw = np.frombuffer(dev.h.read_scratch(off, G * 64), dtype=np.uint64).reshape(G, 8).astype(np.float64)
            us = raw / 100.0 / args.nb
            print(f"stamps3 nt={nt} m={m} G={G}: owner-wave us per column (mean | max)   total {us.sum(1).mean():.2f}")
            for i, nm in enumerate(names[:7]):
                print(f"   {nm:24s} {us[:, i].mean():7.3f} | {us[:, i].max():7.3f}")
        dev.h.set_option("panel_debug", 0)
        dev.h.set_option("panel_nt", 0)
        dev.h.set_option("panel", 3)
    if "xchg" in args.what:
        # floor of the panel's per-column exchange: one all-gather round by store policy and placement
        for mode, nm in ((2, "ping-pong (one-way = half)"), (0, "header all-gather"), (1, "header all-gather + winner row")):
            for G, stride, wt in ((32, 8, False), (32, 8, True), (32, 1, True), (64, 1, True), (32, 1, False)):
                if mode == 2 and G == 64:
                    continue
                us, ids, nf = dev.h.xchg_probe(mode, G, stride, wt, 4000)
                print(f"xchg {nm}: G={G} stride={stride} stores={'sc1' if wt else 'plain'}: {us:.3f} us/round  "
                      f"failures={nf}  xcc ids={sorted(set(ids))} (participant 0 on {ids[0]}, 1 on {ids[1]})", flush=True)
    if "panelx" in args.what or "pstamps" in args.what:
        import numpy as np
        # device-scope pipelined panel (panel=3) / XCD kernel (panel=4)
        variants = (("p3", 3), ("p4", 4))
        dev.h.set_option("panel_nt", 0)
        dev.h.set_option("panel_rt", 4)
        dt = torch.float32 if args.f32 else torch.float64
        for m in (8192, 6000, 4096, 3000, 2048, 1024, 384, 257, 100) if "panelx" in args.what else ():
            for nbw in (args.nb, 100, 17):
                for kind in (gen.U11, gen.INT5):
                    P0 = torch.empty(m, nbw, dtype=dt, device="cuda")
                    dev.fill_(P0, kind, 3)
                    outs = []
                    for nm, mode in variants:
                        dev.h.set_option("panel", mode)
                        P = P0.clone()
                        ipiv = torch.zeros(nbw, dtype=torch.int32, device="cuda")
                        info = torch.zeros(1, dtype=torch.int32, device="cuda")
                        dev.panel_(P, 0, ipiv, info)
                        torch.cuda.synchronize()
                        outs.append((P, ipiv.clone(), int(info.item())))
                    same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
                    print(f"panelx check m={m} jb={nbw} kind={kind}: p4={'same' if same else 'MISMATCH'}(info {outs[1][2]})", flush=True)
        for nm, mode in variants if "panelx" in args.what else ():
            dev.h.set_option("panel", mode)
            for m in (8192, 6144, 4096, 2048, 1024, 256):
                P0 = torch.empty(m, args.nb, dtype=dt, device="cuda")
                dev.fill_(P0, gen.U11, 3)
                ipiv = torch.zeros(args.nb, dtype=torch.int32, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")
                P = P0.clone()

                def run():
                    P.copy_(P0)
                    dev.panel_(P, 0, ipiv, info)
                tmin, tmed = timeit(run, reps=7, warm=2)
                tcopy, _ = timeit(lambda: P.copy_(P0), reps=7, warm=2)
                t = tmin - tcopy
                print(f"panel {nm} m={m} nb={args.nb}: {t * 1e3:.1f} us  ({t * 1e3 / args.nb:.2f} us/col)", flush=True)
        names = ["own: headers+winner", "own: multipliers+granules", "own: update+choose+announce", "own: barrier",
                 "next wave: barrier wait", "next wave: far granules+update", "next wave: publish", "own: second block behind the barrier"]
        dev.h.set_option("panel", 4)
        dev.h.set_option("panel_debug", 1)
        for m in (8192, 4096, 2048, 256, 128):
            rows = 64 * (1 if m <= 2048 else 2 if m <= 4096 else 4 if (m <= 8192 or not args.f32) else 8)
            P = torch.empty(m, args.nb, dtype=dt, device="cuda")
            ipiv = torch.zeros(args.nb, dtype=torch.int32, device="cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")
            for rep in range(2):
                dev.fill_(P, gen.U11, 3)
                dev.panel_(P, 0, ipiv, info)
            torch.cuda.synchronize()
            G = (m + rows - 1) // rows
            need = 256 + 2 * G * 128 + 4 * G * 128 * 16
            off = (need + 255) & ~255
            raw = np.frombuffer(dev.h.read_scratch(off, G * 128), dtype=np.uint64).reshape(G, 16)
            us = raw.astype(np.float64) / 100.0 / args.nb
            tag = f" xcc ids {sorted(set((raw[:, 15] >> 8).tolist()))} same-flag {sorted(set((raw[:, 15] & 1).tolist()))}"
            print(f"stamps4 m={m} G={G}: us per column (mean | max over workgroups)   owner total {us[:, [0, 1, 2, 3, 7]].sum(1).mean():.2f}{tag}")
            for i, nm in enumerate(names[:8]):
                print(f"   {nm:30s} {us[:, i].mean():7.3f} | {us[:, i].max():7.3f}")
            # marks of the launch outside its column loop (PX_TMARK): us after the kernel's entry, wave 0 of each workgroup
            mk = raw[:, [8, 9, 10, 11, 13, 14]].astype(np.float64) / 100.0
            print(f"marks4 m={m} G={G}: us after kernel entry (mean | min | max over workgroups)")
            for i, nm in enumerate(("handshake decided", "tile in registers", "first header shot", "end of column loop",
                                    "scatter issued", "scatter acknowledged")):
                print(f"   {nm:30s} {mk[:, i].mean():8.2f} | {mk[:, i].min():8.2f} | {mk[:, i].max():8.2f}")
            print(f"   outside the loop: before the first shot {mk[:, 2].mean():.2f}, behind the loop {(mk[:, 5] - mk[:, 3]).mean():.2f}")
        dev.h.set_option("panel_debug", 0)
        dev.h.set_option("panel", 3)
    if "cumask" in args.what:
        from collections import Counter
        pats = {
            "no mask": None,
            "bits 0..223": range(0, 224),
            "bits 32..255": range(32, 256),
            "bits i%8!=0": [i for i in range(256) if i % 8 != 0],
            "bits i%8==0": [i for i in range(256) if i % 8 == 0],
            "bits 0..31": range(0, 32),
            "bits i%8==3": [i for i in range(256) if i % 8 == 3],
            "bits 0..127": range(0, 128),
            "bits i%2==0": range(0, 256, 2),
        }
        for nm, bits in pats.items():
            try:
                res = dev.h.cu_mask_probe(bits, 2048)
            except Exception as e:  # noqa: BLE001
                print(f"cumask {nm}: FAILED {e}")
                continue
            xc = Counter(x for x, _ in res)
            cus = Counter((x, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15) for x, hw in res)
            first8 = [x for x, _ in res[:16]]
            print(f"cumask {nm}: blocks per xcc {dict(sorted(xc.items()))}  distinct (xcc,se,sh,cu) {len(cus)}  first blocks' xcc {first8}", flush=True)
    if "lu4" in args.what:
        # whole factorisation: device-scope panel (3) against the XCD-scope panel (4), both drivers; same bits
        dt = torch.float32 if args.f32 else torch.float64
        for n in (args.n,) if args.n != 8192 else (8192, 4096, 12288):
            A0 = torch.empty(n, n, dtype=dt, device="cuda")
            dev.fill_(A0, gen.U11, 1)
            A = A0.clone()
            ipiv = torch.zeros(n, dtype=torch.int32, device="cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")
            ref = None
            for mode, look in ((3, 0), (3, 1), (4, 0), (4, 1)):
                dev.h.set_option("panel", mode)
                dev.h.set_option("lookahead", look)
                dev.h.set_option("lookahead_min", 1024 if look else 0)

                def run():
                    A.copy_(A0)
                    dev.getrf_(A, ipiv, info)
                tmin, _ = timeit(run, reps=5, warm=2)
                tcopy, _ = timeit(lambda: A.copy_(A0), reps=3, warm=1)
                t = tmin - tcopy
                torch.cuda.synchronize()
                if ref is None:
                    ref = (A.clone(), ipiv.clone())
                    same = "reference"
                else:
                    same = "bit-identical" if (torch.equal(ref[0], A) and torch.equal(ref[1], ipiv)) else "MISMATCH"
                dev.h.prof_reset(); dev.h.prof_enable(True); run(); torch.cuda.synchronize()
                dev.h.prof_enable(False)
                pr = dev.h.prof_read()
                print(f"getrf n={n} panel={mode} lookahead={look}: {t:.2f} ms  {2 / 3 * n ** 3 / t / 1e9:.2f} TFLOP/s  info={int(info.item())} {same}  phases "
                      + " ".join(f"{k}={v['ms']:.2f}" for k, v in pr.items() if v['ms'] > 0), flush=True)
        dev.h.set_option("panel", 3); dev.h.set_option("lookahead", 1); dev.h.set_option("lookahead_min", 0)
    if "hyb" in args.what:
        # matrices taller than one XCD holds: shared-CU schedule throughout (hybrid=0) against the hand-over to the
        # XCD-scope driver once the trailing matrix fits (hybrid=1, default); sequential driver as the reference
        dt = torch.float32 if args.f32 else torch.float64
        for n in (args.n,) if args.n != 8192 else (8320, 10240, 12288, 16384):
            A0 = torch.empty(n, n, dtype=dt, device="cuda")
            dev.fill_(A0, gen.U11, 1)
            A = A0.clone()
            ipiv = torch.zeros(n, dtype=torch.int32, device="cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")
            ref = None
            dev.h.set_option("panel", 4)
            for look, hyb in ((0, 1), (1, 0), (1, 1)):
                dev.h.set_option("lookahead", look)
                dev.h.set_option("hybrid", hyb)

                def run():
                    A.copy_(A0)
                    dev.getrf_(A, ipiv, info)
                tmin, _ = timeit(run, reps=4, warm=2)
                tcopy, _ = timeit(lambda: A.copy_(A0), reps=3, warm=1)
                t = tmin - tcopy
                torch.cuda.synchronize()
                if ref is None:
                    ref = (A.clone(), ipiv.clone())
                    same = "reference"
                else:
                    same = "bit-identical" if (torch.equal(ref[0], A) and torch.equal(ref[1], ipiv)) else "MISMATCH"
                print(f"getrf n={n} lookahead={look} hybrid={hyb}: {t:.2f} ms  {2 / 3 * n ** 3 / t / 1e9:.2f} TFLOP/s  info={int(info.item())} {same}", flush=True)
            del A0, A
        dev.h.set_option("lookahead", 1); dev.h.set_option("hybrid", 1)
    if "pmc" in args.what:
        # workload for `rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE`: two kernels of known byte counts
        # (calibration) followed by the trailing-update kernel at LU-like shapes
        m = 8064
        Cm = torch.empty(m, m, dtype=torch.float64, device="cuda")
        dev.fill_(Cm, gen.U11, 1)                   # lsx fill_kernel: writes m*m*8 B (8 B per lane)
        Cc = Cm.clone()                             # torch copy: reads m*m*8 B, writes m*m*8 B
        dev.h.set_option("gemm_waves", 0)
        for k in (128, 256):
            A = torch.randn(m, k, dtype=torch.float64, device="cuda")
            B = torch.randn(k, m, dtype=torch.float64, device="cuda")
            dev.gemm_sub_(Cm, A, B)                 # algorithmic: read + write C = 2*m*m*8 B (+ A, B slabs)
        torch.cuda.synchronize()
        print(f"pmc workload done: m={m}, C bytes one way = {m * m * 8}")
    if "pmcpanel" in args.what:
        # workload for `rocprofv3 --pmc FETCH_SIZE|WRITE_SIZE`: a copy of known size (calibration), then the
        # XCD-scope panel kernel on a 8192 x 128 panel (algorithmic: read + write the panel once = 2 * 8192 * 128 * 8 B)
        m = 8192
        dev.h.set_option("panel", 4)
        big = torch.empty(m, m, dtype=torch.float64, device="cuda")
        dev.fill_(big, gen.U11, 1)
        bigc = big.clone()                          # calibration: reads and writes m*m*8 bytes
        P = torch.empty(m, args.nb, dtype=torch.float64, device="cuda")
        ipiv = torch.zeros(args.nb, dtype=torch.int32, device="cuda")
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        for rep in range(3):
            dev.fill_(P, gen.U11, 3 + rep)
            dev.panel_(P, 0, ipiv, info)
        torch.cuda.synchronize()
        print(f"pmcpanel workload done: panel {m} x {args.nb}, bytes one way = {m * args.nb * 8}; calibration copy {m * m * 8} one way")
    if "trsvt" in args.what:
        # few-right-hand-side solves from the factors: transposed (one launch per 128-row step) against the plain
        # solve in the same form (trsv=0: it streams the same n^2 elements once per sweep) and in its default form
        HBM = 8.0e12   # bytes / s (MI355X data sheet)
        for dt in (torch.float64, torch.float32):
            for n in (1024, 4096, 8192):
                A = torch.empty(n, n, dtype=dt, device="cuda")
                dev.fill_(A, gen.U11, 1)
                ipiv, info = dev.getrf_(A)
                for nrhs in (1, 8):
                    B0 = torch.empty(n, nrhs, dtype=dt, device="cuda")
                    dev.fill_(B0, gen.U11, 2)
                    B = B0.clone()
                    res = {}
                    for rnd in range(2):          # two alternating rounds: the spread of the same command
                        for name, trans, mode in (("transposed", True, 2), ("plain trsv=0", False, 0), ("plain trsv=2", False, 2)):
                            dev.h.set_option("trsv", mode)
                            res.setdefault(name, []).append(timeit(lambda: dev.getrs_(A, ipiv, B, trans=trans), reps=21, warm=3)[1])
                    dev.h.set_option("trsv", 2)
                    by = A.element_size() * float(n) * n
                    print(f"solve {str(dt)[6:]} n={n} nrhs={nrhs}: " + "  ".join(
                        f"{k} {min(v) * 1e3:.1f} us (rounds {v[0] * 1e3:.1f} / {v[1] * 1e3:.1f}; {by / min(v) / 1e-3 / HBM * 100:.1f} % of HBM)"
                        for k, v in res.items()), flush=True)
    if "getrs_t" in args.what:
        # many right-hand sides: the transposed solve in groups of 8 columns (getrs_t_blocked_min = 0), its blocked
        # sweeps on the TN form of the MFMA tile (= 1), and the plain solve of the same shape -- the same flops on
        # the same tile with the NN kernel: the yardstick.  Medians of two alternating rounds, the copy that restores
        # the right-hand sides subtracted.
        dt = torch.float64
        for n in (1024, 4096, 8192):
            A = torch.empty(n, n, dtype=dt, device="cuda")
            dev.fill_(A, gen.U11, 1)
            ipiv, info = dev.getrf_(A)
            for nrhs in (8, 16, 32, 64, 128, 256, 1024):
                B0 = torch.empty(n, nrhs, dtype=dt, device="cuda")
                dev.fill_(B0, gen.U11, 2)
                B = B0.clone()
                reps = 5 if n * nrhs >= 4096 * 256 else 11
                res, paths = {}, {}
                for rnd in range(2):
                    t_copy = timeit(lambda: B.copy_(B0), reps=reps, warm=1)[1]
                    for name, trans, opt in (("grouped", True, 0), ("blocked", True, 1), ("plain", False, None)):
                        if opt is not None:
                            dev.h.set_option("getrs_t_blocked_min", opt)

                        def run():
                            B.copy_(B0)
                            dev.getrs_(A, ipiv, B, trans=trans)
                        res.setdefault(name, []).append(timeit(run, reps=reps, warm=1)[1] - t_copy)
                        if trans:
                            paths[name] = dev.h.get_option("getrs_t_path")
                assert paths == {"grouped": 0, "blocked": 1}, paths
                g, b, pl = (min(res[k]) for k in ("grouped", "blocked", "plain"))
                fl = 2.0 * n * n * nrhs
                print(f"getrs_t f64 n={n} nrhs={nrhs}: grouped {g:.3f} ms  blocked {b:.3f} ms ({fl / b / 1e9:.1f} TFLOP/s)  "
                      f"plain {pl:.3f} ms  | grouped/blocked {g / b:.2f}  blocked/plain {b / pl:.2f}  "
                      f"(rounds: grouped {res['grouped'][0]:.3f}/{res['grouped'][1]:.3f} blocked {res['blocked'][0]:.3f}/"
                      f"{res['blocked'][1]:.3f} plain {res['plain'][0]:.3f}/{res['plain'][1]:.3f})", flush=True)
        dev.h.set_option("getrs_t_blocked_min", 64)
    if "potrf" in args.what:
        # Cholesky beside LU on the SAME symmetric positive definite matrix, same process: medians of two alternating
        # rounds, the copy that restores the matrix timed on its own and subtracted.  Then one profiled factorisation
        # for the split: diagonal block (panel), block row (trsm), trailing update (gemm).
        for dt in (torch.float64, torch.float32):
            for n in (4096, 8192):
                G = torch.empty(n, n, dtype=dt, device="cuda")
                dev.fill_(G, gen.U11, 1)
                A0 = G @ G.t() / n + torch.eye(n, dtype=dt, device="cuda")   # plumbing: builds the input only
                del G
                A = A0.clone()
                ipiv = torch.empty(n, dtype=torch.int32, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")
                res = {}
                for rnd in range(2):
                    t_copy = timeit(lambda: A.copy_(A0), reps=7, warm=2)[1]

                    def chol():
                        A.copy_(A0)
                        dev.potrf_(A, info)

                    def lu():
                        A.copy_(A0)
                        dev.getrf_(A, ipiv, info)
                    for name, fn in (("potrf", chol), ("getrf", lu)):
                        res.setdefault(name, []).append(timeit(fn, reps=7, warm=2)[1] - t_copy)
                        assert int(info.item()) == 0, (name, int(info.item()))
                pf, gf = min(res["potrf"]), min(res["getrf"])
                dev.h.prof_enable(True)
                split = []
                for _ in range(2):                      # the second pass is the warm one
                    A.copy_(A0)
                    torch.cuda.synchronize()
                    dev.h.prof_reset()
                    dev.potrf_(A, info)
                    dev.h.synchronize()
                    split = dev.h.prof_read()
                dev.h.prof_enable(False)
                tot = sum(v["ms"] for v in split.values()) or 1.0
                nd = max(split["panel"]["launches"], 1)
                print(f"potrf {str(dt)[6:]} n={n}: potrf {pf:.3f} ms ({n ** 3 / 3 / pf / 1e9:.1f} TFLOP/s)  getrf {gf:.3f} ms  "
                      f"| potrf/getrf {pf / gf:.3f}  (rounds: potrf {res['potrf'][0]:.3f}/{res['potrf'][1]:.3f} getrf "
                      f"{res['getrf'][0]:.3f}/{res['getrf'][1]:.3f}; copy {t_copy:.3f})", flush=True)
                print(f"    profiled pass: diagonal {split['panel']['ms']:.3f} ms / {split['panel']['launches']} launches = "
                      f"{split['panel']['ms'] / nd * 1e3:.1f} us each;  strip {split['trsm']['ms']:.3f} ms / "
                      f"{split['trsm']['launches']};  update {split['gemm']['ms']:.3f} ms / {split['gemm']['launches']} "
                      f"({split['gemm']['ms'] / tot * 100:.0f} % of the bracketed time, "
                      f"{split['gemm']['flops'] / max(split['gemm']['ms'], 1e-9) / 1e9:.1f} TFLOP/s)", flush=True)
                del A, A0
    if "potri" in args.what:
        # The SPD inverse beside the LU inverse of the SAME matrix G G^T / n + I, one process: potrf + potri against
        # getrf + getri, medians of two alternating rounds with the restoring copy timed on its own and subtracted;
        # then the trapezoid product V^T V alone in both tile orders (0: deepest first, 1: the symmetric update's).
        for dt in (torch.float64, torch.float32):
            for n in (2048, 4096, 8192):
                G = torch.empty(n, n, dtype=dt, device="cuda")
                dev.fill_(G, gen.U11, 1)
                A0 = G @ G.t() / n + torch.eye(n, dtype=dt, device="cuda")   # plumbing: builds the input only
                del G
                A = A0.clone()
                Inv = torch.empty_like(A)
                ipiv = torch.empty(n, dtype=torch.int32, device="cuda")
                info = torch.zeros(1, dtype=torch.int32, device="cuda")
                res = {}
                for rnd in range(2):
                    t_copy = timeit(lambda: A.copy_(A0), reps=5, warm=2)[1]

                    def chol():
                        A.copy_(A0)
                        dev.potrf_(A, info)
                        dev.potri_(A, info)

                    def chol_f():
                        A.copy_(A0)
                        dev.potrf_(A, info)

                    def lu():
                        A.copy_(A0)
                        dev.getrf_(A, ipiv, info)
                        dev.getri(A, ipiv, Inv)
                    for name, fn in (("potrf+potri", chol), ("potrf", chol_f), ("getrf+getri", lu)):
                        res.setdefault(name, []).append(timeit(fn, reps=5, warm=2)[1] - t_copy)
                        assert int(info.item()) == 0, (name, int(info.item()))
                pi, pf, gi = (min(res[k]) for k in ("potrf+potri", "potrf", "getrf+getri"))
                print(f"potri {str(dt)[6:]} n={n}: potrf+potri {pi:.3f} ms ({n ** 3 / pi / 1e9:.1f} TFLOP/s of n^3; potrf {pf:.3f}, "
                      f"potri {pi - pf:.3f})  getrf+getri {gi:.3f} ms  | Cholesky/LU {pi / gi:.3f}  (rounds: "
                      f"{res['potrf+potri'][0]:.3f}/{res['potrf+potri'][1]:.3f} against {res['getrf+getri'][0]:.3f}/"
                      f"{res['getrf+getri'][1]:.3f}; copy {t_copy:.3f})", flush=True)
                V = torch.tril(A0)                      # any lower-triangular operand times the same
                Cm = torch.zeros_like(A0)
                t_ord = {}
                dev.h.set_option("lauum_descending", 1)      # the k-slab order potri runs
                for rnd in range(2):
                    for order in (0, 1):
                        dev.h.set_option("potri_order", order)
                        t_ord.setdefault(order, []).append(timeit(lambda: dev.lauum_tn_(Cm, V), reps=7, warm=2)[1])
                dev.h.set_option("potri_order", 0)
                dev.h.set_option("lauum_descending", 0)
                t_asc = timeit(lambda: dev.lauum_tn_(Cm, V), reps=7, warm=2)[1]
                t0, t1 = min(t_ord[0]), min(t_ord[1])
                print(f"    V^T V alone, {dev.h.get_option('potri_tiles')} tiles: deepest first {t0:.3f} ms ({n ** 3 / 3 / t0 / 1e9:.1f} "
                      f"TFLOP/s of n^3/3)  update order {t1:.3f} ms  | deepest/update {t0 / t1:.3f}  (rounds: "
                      f"{t_ord[0][0]:.3f}/{t_ord[0][1]:.3f} against {t_ord[1][0]:.3f}/{t_ord[1][1]:.3f}; k ascending, deepest first: "
                      f"{t_asc:.3f} ms)", flush=True)
                del A, A0, Inv, V, Cm
    if "posx" in args.what:
        # Condition estimate and error bounds of the Cholesky family beside their LU counterparts on the SAME matrix
        # G G^T / n + I, one process, medians of 7 after warm-up:
        #   the symmetric residual pass against the general one (GB/s of the bytes each actually reads of A),
        #   lsx_potrs_* at nrhs = 1 with potrs_few_max = 0 (block sweeps) and 8 (step kernels),
        #   pocon against gecon on the LU factors, porfs against gerfs at nrhs = 1 and 8.
        med = lambda fn: timeit(fn, reps=7, warm=2)[1]   # noqa: E731
        for dt in (torch.float64, torch.float32):
            sfx, es = ("f64", 8) if dt == torch.float64 else ("f32", 4)
            for n in (4096, 8192):
                G = torch.empty(n, n, dtype=dt, device="cuda")
                dev.fill_(G, gen.U11, 1)
                A = G @ G.t() / n + torch.eye(n, dtype=dt, device="cuda")   # plumbing: builds the input only
                del G
                XT = torch.empty(n, 8, dtype=dt, device="cuda")
                dev.fill_(XT, gen.U11, 2)
                B = A @ XT
                R, W = torch.empty_like(B), torch.empty_like(B)
                hook_sym = getattr(dev.lib, f"lsx_diag_resid_bound_sym_{sfx}_dev")
                hook_gen = getattr(dev.lib, f"lsx_diag_resid_bound_{sfx}_dev")
                for nr in (1, 8):
                    ts = med(lambda: hook_sym(dev.h.ptr, n, nr, A.data_ptr(), n, B.data_ptr(), 8, XT.data_ptr(), 8,
                                              R.data_ptr(), W.data_ptr(), 8))
                    tg = med(lambda: hook_gen(dev.h.ptr, 0, n, nr, A.data_ptr(), n, B.data_ptr(), 8, XT.data_ptr(), 8,
                                              R.data_ptr(), W.data_ptr(), 8))
                    print(f"posx {sfx} n={n} resid NR={nr}: symmetric {ts * 1e3:.1f} us ({es * n * (n + 1) / 2 / ts / 1e6:.0f} GB/s "
                          f"of n(n+1)/2 elements)  general {tg * 1e3:.1f} us ({es * n * n / tg / 1e6:.0f} GB/s of n^2)  "
                          f"| symmetric/general {ts / tg:.2f}", flush=True)
                U = A.clone()
                info = dev.potrf_(U)
                LU = A.clone()
                ipiv, linfo = dev.getrf_(LU)
                assert int(info.item()) == 0 and int(linfo.item()) == 0
                x = torch.empty(n, 1, dtype=dt, device="cuda")
                tp = {}
                for few in (0, 8):
                    dev.h.set_option("potrs_few_max", few)

                    def solve1():
                        x.copy_(B[:, :1])
                        dev.potrs_(U, x)
                    tp[few] = med(solve1)
                    assert dev.h.get_option("potrs_path") == (1 if few else 0)
                dev.h.set_option("potrs_few_max", 0)

                def lusolve1():
                    x.copy_(B[:, :1])
                    dev.getrs_(LU, ipiv, x)
                tl = med(lusolve1)
                print(f"posx {sfx} n={n} potrs nrhs=1: sweeps {tp[0] * 1e3:.1f} us  step kernels {tp[8] * 1e3:.1f} us  "
                      f"| steps/sweeps {tp[8] / tp[0]:.2f}   (getrs nrhs=1: {tl * 1e3:.1f} us)", flush=True)
                anorm = float(dev.norm_sym(A).item())
                t0 = time.perf_counter()
                reps = 5
                for _ in range(reps):
                    rp = dev.pocon(U, anorm)
                tpo = (time.perf_counter() - t0) / reps * 1e3
                sp = dev.h.get_option("pocon_solves")
                t0 = time.perf_counter()
                for _ in range(reps):
                    rg = dev.rcond(LU, ipiv, anorm, 1)
                tge = (time.perf_counter() - t0) / reps * 1e3
                sg = dev.h.get_option("gecon_solves")
                print(f"posx {sfx} n={n} pocon {tpo:.3f} ms ({sp} solves, rcond {rp:.3e})  gecon {tge:.3f} ms ({sg} solves, "
                      f"rcond {rg:.3e})  | pocon/gecon {tpo / tge:.2f}  (host wall clock, both synchronise)", flush=True)
                for nr in (1, 8):
                    Bk = B[:, :nr].contiguous()
                    X0 = Bk.clone()
                    dev.potrs_(U, X0)
                    sgn = torch.where(torch.arange(n, device="cuda") % 2 == 0, 1 + 2.0 ** -10, 1 - 2.0 ** -10).to(dt)
                    X0 = X0 * sgn[:, None]                    # the tests' perturbed start: one to three steps
                    X = X0.clone()
                    tt = {}
                    for name in ("porfs", "gerfs"):
                        ts_ = []
                        for _ in range(reps + 1):
                            X.copy_(X0)
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            if name == "porfs":
                                dev.porfs_(A, U, Bk, X)
                            else:
                                dev.gerfs_(A, LU, ipiv, Bk, X)
                            ts_.append((time.perf_counter() - t0) * 1e3)
                        tt[name] = sorted(ts_[1:])[len(ts_[1:]) // 2]
                        tt[name + "_steps"] = dev.h.get_option(name + "_steps")
                        tt[name + "_solves"] = dev.h.get_option(name + "_solves")
                    print(f"posx {sfx} n={n} nrhs={nr}: porfs {tt['porfs']:.3f} ms ({tt['porfs_steps']} steps, "
                          f"{tt['porfs_solves']} estimator solves)  gerfs {tt['gerfs']:.3f} ms ({tt['gerfs_steps']} steps, "
                          f"{tt['gerfs_solves']} solves)  | porfs/gerfs {tt['porfs'] / tt['gerfs']:.2f}", flush=True)
                del A, U, LU, B, XT, R, W
    if "gecon" in args.what:
        # the condition estimate beside the factorisation it follows (fp64, 1-norm; medians)
        for n in (1024, 4096, 8192):
            A0 = torch.empty(n, n, dtype=torch.float64, device="cuda")
            dev.fill_(A0, gen.U11, 1)
            A = A0.clone()
            ipiv = torch.zeros(n, dtype=torch.int32, device="cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")

            def factor():
                A.copy_(A0)
                dev.getrf_(A, ipiv, info)
            t_lu = timeit(factor, reps=7, warm=2)[1] - timeit(lambda: A.copy_(A0), reps=7, warm=2)[1]
            factor()                      # the copy timing left the unfactored matrix in A
            t_nrm = timeit(lambda: dev.norm(A0, 1), reps=11, warm=2)[1]
            anorm = float(dev.norm(A0, 1).item())
            for _ in range(2):
                rc = dev.rcond(A, ipiv, anorm)
            ts = []
            for _ in range(9):            # synchronous call: host clock around it
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = dev.rcond(A, ipiv, anorm)
                ts.append((time.perf_counter() - t0) * 1e3)
            t_con = sorted(ts)[len(ts) // 2]
            print(f"gecon f64 n={n}: getrf {t_lu:.3f} ms  lange {t_nrm:.3f} ms  gecon {t_con:.3f} ms "
                  f"({dev.h.get_option('gecon_solves')} solves, {t_con / t_lu * 100:.1f} % of getrf)  rcond {rc:.3e}", flush=True)
    if "gerfs" in args.what:
        # the residual-and-bound pass of the refined solve (kernels_refine.hip) alone, plain and transposed, beside the
        # fp32-in / fp64-sum residual of the mixed-precision solve on the same fp32 data; then a whole gerfs call beside
        # the factorisation and the condition estimate.  Median of 21 timed calls after 3 warm-up calls, two
        # alternating rounds (the smaller median is reported, both are printed).
        HBM = 8.0e12
        lib, hp = dev.lib, dev.h.ptr

        def med(fn):
            return timeit(fn, reps=21, warm=3)[1]
        for n in (1024, 4096, 8192):
            for dt in (torch.float64, torch.float32):
                sfx = "f64" if dt == torch.float64 else "f32"
                A = torch.empty(n, n, dtype=dt, device="cuda")
                dev.fill_(A, gen.U11, 1)
                for nrhs in (1, 8):
                    B = torch.empty(n, nrhs, dtype=dt, device="cuda")
                    X = torch.empty(n, nrhs, dtype=dt, device="cuda")
                    dev.fill_(B, gen.U11, 2)
                    dev.fill_(X, gen.U11, 3)
                    R, W = torch.empty_like(B), torch.empty_like(B)
                    fn = getattr(lib, f"lsx_diag_resid_bound_{sfx}_dev")
                    runs = {"plain": lambda: fn(hp, 0, n, nrhs, A.data_ptr(), n, B.data_ptr(), nrhs, X.data_ptr(), nrhs,
                                                R.data_ptr(), W.data_ptr(), nrhs),
                            "transposed": lambda: fn(hp, 1, n, nrhs, A.data_ptr(), n, B.data_ptr(), nrhs, X.data_ptr(), nrhs,
                                                     R.data_ptr(), W.data_ptr(), nrhs)}
                    if dt == torch.float32:
                        X64 = X.double()
                        runs["resid_mixed"] = lambda: lib.lsx_diag_resid_mixed_dev(hp, n, nrhs, A.data_ptr(), n, B.data_ptr(),
                                                                                   nrhs, X64.data_ptr(), nrhs, R.data_ptr(), nrhs)
                    for k, f in runs.items():       # a refused call must not be timed as a very fast pass
                        N.check(f(), k)
                    res = {k: [] for k in runs}
                    for _ in range(2):
                        for k, f in runs.items():
                            res[k].append(med(f))
                    by = float(n) * n * A.element_size()
                    print(f"resid_bound {sfx} n={n} nrhs={nrhs}: " + "  ".join(
                        f"{k} {min(v) * 1e3:.1f} us (rounds {v[0] * 1e3:.1f} / {v[1] * 1e3:.1f}; "
                        f"{by / (min(v) * 1e-3) / HBM * 100:.1f} % of 8 TB/s)" for k, v in res.items()), flush=True)
        for n in (1024, 4096, 8192):
            A0 = torch.empty(n, n, dtype=torch.float64, device="cuda")
            dev.fill_(A0, gen.U11, 1)
            LU = A0.clone()
            ipiv = torch.zeros(n, dtype=torch.int32, device="cuda")
            info = torch.zeros(1, dtype=torch.int32, device="cuda")

            def factor():
                LU.copy_(A0)
                dev.getrf_(LU, ipiv, info)
            t_lu = timeit(factor, reps=7, warm=2)[1] - timeit(lambda: LU.copy_(A0), reps=7, warm=2)[1]
            factor()
            anorm = float(dev.norm(A0, 1).item())

            def host_med(fn, reps=21, warm=3):      # synchronous calls: host clock around them
                for _ in range(warm):
                    fn()
                ts = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                return sorted(ts)[len(ts) // 2]
            t_con = host_med(lambda: dev.rcond(LU, ipiv, anorm))
            for nrhs in (1, 8):
                B = torch.empty(n, nrhs, dtype=torch.float64, device="cuda")
                dev.fill_(B, gen.U11, 2)
                X0 = B.clone()
                dev.getrs_(LU, ipiv, X0)
                X = X0.clone()

                def refine():
                    X.copy_(X0)
                    return dev.gerfs_(A0, LU, ipiv, B, X)
                rounds = [host_med(refine) for _ in range(2)]
                ferr, berr = refine()
                print(f"gerfs f64 n={n} nrhs={nrhs}: getrf {t_lu:.3f} ms  gecon {t_con:.3f} ms  gerfs {min(rounds):.3f} ms "
                      f"(rounds {rounds[0]:.3f} / {rounds[1]:.3f}; {dev.h.get_option('gerfs_steps')} steps, "
                      f"{dev.h.get_option('gerfs_solves')} estimator solves, {min(rounds) / t_lu * 100:.1f} % of getrf)  "
                      f"berr {berr.max():.2e} ferr {ferr.max():.2e}", flush=True)
    if "equil" in args.what:
        # equilibration (kernels_equil.hip): each pass of geequ beside the lange call that reads the same bytes -- the row
        # pass beside the infinity-norm, the column pass beside the 1-norm -- then laqge, and a whole gesvx with its share
        # spent on equilibration.  Median of 21 timed calls after 3 warm-up calls, two alternating rounds (the smaller
        # median is reported, both are printed); gesvx synchronises, so it is timed with the host clock.
        HBM = 8.0e12
        lib, hp = dev.lib, dev.h.ptr

        def med(fn):
            return timeit(fn, reps=21, warm=3)[1]
        for n in (4096, 8192):
            for dt in (torch.float64, torch.float32):
                sfx = "f64" if dt == torch.float64 else "f32"
                # the recipe of tests/cpu_refine.scaled_system: columns 2^-30 .. 2^30, every third row 2^-20
                A64 = torch.empty(n, n, dtype=torch.float64, device="cuda")
                dev.fill_(A64, gen.U11, 1)
                torch.cuda.synchronize()
                scales = torch.randint(-30, 31, (n,), generator=torch.Generator().manual_seed(n)).double()
                A64 *= (2.0 ** scales).cuda()[None, :]
                A64[::3] *= 2.0 ** -20
                A0 = A64.to(dt)
                del A64
                A = A0.clone()
                r, c = torch.empty(n, dtype=dt, device="cuda"), torch.empty(n, dtype=dt, device="cuda")
                st, out = torch.zeros(4, dtype=torch.float64, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda")
                gp = getattr(lib, f"lsx_diag_geequ_pass_{sfx}_dev")
                ln = getattr(lib, f"lsx_lange_{sfx}_dev")
                runs = {"row pass": lambda: gp(hp, 1, n, n, A0.data_ptr(), n, r.data_ptr(), c.data_ptr(), st.data_ptr()),
                        "lange inf": lambda: ln(hp, N.NORM_INF, n, n, A0.data_ptr(), n, out.data_ptr()),
                        "column pass": lambda: gp(hp, 2, n, n, A0.data_ptr(), n, r.data_ptr(), c.data_ptr(), st.data_ptr()),
                        "lange one": lambda: ln(hp, N.NORM_ONE, n, n, A0.data_ptr(), n, out.data_ptr()),
                        "geequ": lambda: gp(hp, 3, n, n, A0.data_ptr(), n, r.data_ptr(), c.data_ptr(), st.data_ptr())}
                for k, f in runs.items():           # a refused call must not be timed as a very fast pass
                    N.check(f(), k)
                res = {k: [] for k in runs}
                for _ in range(2):
                    for k, f in runs.items():
                        res[k].append(med(f))
                rowcnd, colcnd, amax, ginfo = st.tolist()
                by = float(n) * n * A0.element_size()
                print(f"geequ {sfx} n={n}: " + "  ".join(
                    f"{k} {min(v) * 1e3:.1f} us (rounds {v[0] * 1e3:.1f} / {v[1] * 1e3:.1f}; "
                    f"{(2 if k == 'geequ' else 1) * by / (min(v) * 1e-3) / HBM * 100:.1f} % of 8 TB/s)" for k, v in res.items())
                    + f"  row / inf {min(res['row pass']) / min(res['lange inf']):.2f}  column / one "
                      f"{min(res['column pass']) / min(res['lange one']):.2f}", flush=True)

                def scale():
                    A.copy_(A0)
                    return dev.laqge_(A, r, c, rowcnd, colcnd, amax)
                t_copy = min(med(lambda: A.copy_(A0)) for _ in range(2))
                t_laq = min(med(scale) for _ in range(2)) - t_copy
                print(f"laqge {sfx} n={n}: {t_laq * 1e3:.1f} us (equed {scale()}; read + write "
                      f"{2 * by / (t_laq * 1e-3) / HBM * 100:.1f} % of 8 TB/s; the copy that resets the matrix "
                      f"{t_copy * 1e3:.1f} us is subtracted)", flush=True)
                B0 = torch.empty(n, 1, dtype=dt, device="cuda")
                dev.fill_(B0, gen.U11, 2)
                B = B0.clone()
                LU, X = torch.empty(n, n, dtype=dt, device="cuda"), torch.empty(n, 1, dtype=dt, device="cuda")

                def host_med(fn, reps=7, warm=2):
                    for _ in range(warm):
                        fn()
                    ts = []
                    for _ in range(reps):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    return sorted(ts)[len(ts) // 2]

                def driver(equil):
                    A.copy_(A0)
                    B.copy_(B0)
                    return dev.gesvx_(A, B, equilibrate=equil, LU=LU, X=X)
                t_e, t_n = host_med(lambda: driver(True)), host_med(lambda: driver(False))
                o = driver(True)
                t_eq = min(res["geequ"]) + t_laq
                print(f"gesvx {sfx} n={n} nrhs=1: equilibrated {t_e:.3f} ms (equed {o['equed']}, rcond {o['rcond']:.2e}, berr "
                      f"{o['berr'][0]:.1e}), fact='N' {t_n:.3f} ms; geequ + laqge {t_eq:.3f} ms = {t_eq / t_e * 100:.1f} % of "
                      f"the equilibrated call", flush=True)
    if "lu" in args.what:
        n = args.n
        A0 = torch.empty(n, n, dtype=torch.float32 if args.f32 else torch.float64, device="cuda")
        dev.fill_(A0, gen.U11, 1)
        A = A0.clone()
        ipiv = torch.zeros(n, dtype=torch.int32, device="cuda")
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        dev.h.set_option("panel_nt", 0)
        dev.h.set_option("gemm_waves", 0)
        for mode, rt, look, nb, kb in ((3, 4, 0, 128, 1), (3, 4, 2, 128, 1), (3, 4, 1, 128, 1), (3, 4, 0, 128, 2), (3, 4, 0, 64, 1), (3, 4, 0, 96, 1), (4, 4, 0, 128, 1), (4, 4, 1, 128, 1)):
            if True:
                dev.h.set_option("kblock", kb)
                dev.h.set_option("panel", mode)
                dev.h.set_option("panel_rt", rt)
                dev.h.set_option("lookahead", look)
                dev.h.set_option("nb", nb)

                def run():
                    A.copy_(A0)
                    dev.getrf_(A, ipiv, info)
                tmin, _ = timeit(run, reps=3, warm=1)
                tcopy, _ = timeit(lambda: A.copy_(A0), reps=3, warm=1)
                t = tmin - tcopy
                dev.h.prof_reset(); dev.h.prof_enable(True); run(); torch.cuda.synchronize()
                dev.h.prof_enable(False)
                pr = dev.h.prof_read()
                print(f"getrf n={n} panel={mode} rt={rt} lookahead={look} nb={nb} kblock={kb}: {t:.2f} ms  {2 / 3 * n ** 3 / t / 1e9:.2f} TFLOP/s  phases "
                      + " ".join(f"{k}={v['ms']:.2f}" for k, v in pr.items()), flush=True)
        dev.h.set_option("kblock", 1); dev.h.set_option("panel", 4); dev.h.set_option("lookahead", 1)
        dev.h.set_option("nb", 128)


if __name__ == "__main__":
    main()
