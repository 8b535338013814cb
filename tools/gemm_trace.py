"""s_memtime trace of gemm_c8_pf_kernel's stage body (wave 0 of blocks 0..3) at the fc6 and fc7 shapes of the headline, in the folding
form the pipelines launch (row_invariant = 1): cycles per 16-MFMA chunk against the 1024 of 16 back-to-back v_mfma_f32_32x32x2f32, the
lgkmcnt(0) and vmcnt(0) + s_barrier waits at the stage boundary, and the block's prologue / K loop / epilogue.  The stamped kernel is an
instantiation of its own in the debug flavour (libmpn_hip_dbg.so); s_memtime counts shader cycles on gfx950.

Per traced stage the kernel records [start, chunk 1 / 2 / 3 start - start, before the lgkmcnt(0) - start, lgkmcnt(0) wait, vmcnt(0) +
barrier wait]; the last chunk's own cycles are the next stage's start minus its start minus the two waits (a fold of the accumulator at a
K-segment boundary lands in that figure: the medians ignore it)."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import multipathnet_amd
lib = multipathnet_amd._lib.load("debug")
NST, REC = 64, 8
buf = torch.zeros(4 * NST * REC + 16, dtype=torch.int64, device="cuda")
lib.mpn_debug_set_gemm_trace(C.c_void_p(buf.data_ptr()))


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


for name, (M, K, N) in (("fc6", (1000, 25088, 4096)), ("fc7", (1000, 4096, 4096))):
    buf.zero_()
    ms = C.c_float()
    rc = lib.mpn_debug_bench_linear_ri(M, K, N, 1, 3, C.byref(ms))
    torch.cuda.synchronize()
    if rc != 0:
        raise SystemExit("mpn_debug_bench_linear_ri failed (%d): %s" % (rc, lib.mpn_last_error().decode()))
    h = buf.cpu()
    st = h[:4 * NST * REC].view(4, NST, REC)
    ph = h[4 * NST * REC:].view(4, 4)
    print("%s %d x %d x %d: %.1f us/launch (stamped kernel)" % (name, M, K, N, ms.value * 1e3))
    for b in range(4):
        rows = [r for r in st[b].tolist() if r[0] != 0]
        if len(rows) < 3:
            continue
        recs = []
        for r, nxt in zip(rows[:-1], rows[1:]):
            total = nxt[0] - r[0]
            recs.append((r[1], r[2] - r[1], r[3] - r[2], total - r[3] - r[5] - r[6], r[4] - r[3], r[5], r[6], total))
        print(" block %d: %d stages of %d traced; prologue %d, K loop %d, epilogue issue %d cycles" % (b, len(rows), ph[b][3], ph[b][0], ph[b][1], ph[b][2]))
        print("   median per stage: chunks %s (1024 = 16 bare MFMAs), stamp -> lgkmcnt(0) %d, lgkmcnt(0) wait %d, vmcnt(0) + barrier wait %d, stage %d (4096 bare)" % (
            " ".join(str(med([r[i] for r in recs])) for i in range(4)), med([r[4] for r in recs]), med([r[5] for r in recs]), med([r[6] for r in recs]),
            med([r[7] for r in recs])))
        print("   K loop / stages: %.1f cycles per stage, %.2f per MFMA" % (ph[b][1] / max(1, ph[b][3]), ph[b][1] / max(1, ph[b][3]) / 64.0))
        print("   first stages [chunk0 chunk1 chunk2 chunk3 | lgkm wait, vm+barrier wait | stage]: " +
              " ".join("[%d %d %d %d | %d %d | %d]" % (r[0], r[1], r[2], r[3], r[5], r[6], r[7]) for r in recs[:6]))
lib.mpn_debug_set_gemm_trace(None)
