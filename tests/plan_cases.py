"""The plan predictors over every autotuner candidate: the rows that pin the GEMM dispatch across refactors.

``rows(lib)`` yields ``(key, value)`` for ``gemm_partial_slabs``, ``gemm_plan`` (the pair installed in the tuned table)
and ``gemm_f8f8_partial_slabs`` over M x shapes x candidates x workspace sizes. ``python tests/plan_cases.py OUT``
writes them all, one ``key = value`` line each (two builds agree when the files are equal); ``--thin`` writes the
sample kept as tests/golden/gemm_plan_rows.txt: every M x shape, and per M x shape a stride of the candidates chosen
so that every hint bit, every tile code and every workspace size appears."""
import sys

MS = (1, 16, 17, 32, 64, 65, 128, 256, 512, 8192)
# (N, K, glu, fp8)
SHAPES = ((12288, 4096, False, False), (22016, 4096, True, False), (4096, 11008, False, False),
          (4096, 1376, False, False), (6400, 1600, False, False), (1600, 6400, False, False),
          (10240, 8192, False, True), (96, 72, False, False), (48, 64, False, False))
WS = (4 * (64 << 20), 1 << 20, 0)
F8_SPLITS = (0, 1, 2, 3, 8)


def pairs(A, M, N, K, glu, fp8):
    out = [(0, 0)] + list(A.candidates(M, N, K, glu, fp8))
    for neox in (False, True):
        out += A.qkv_epi_candidates(M, N, K, 128, neox)
    return list(dict.fromkeys(out))


def rows(lib, A, thin=False):
    for M in MS:
        for N, K, glu, fp8 in SHAPES:
            ps = pairs(A, M, N, K, glu, fp8)
            step = max(1, len(ps) // 10) if thin else 1
            for i, (nt, s) in enumerate(ps):
                # the thinned sample: a stride, offset per (M, shape) so that the strides together reach every
                # candidate position, plus the first and last pair
                if thin and i not in (0, len(ps) - 1) and (i + M + N) % step and nt & ~(1 << 20) != 4 << 8:
                    continue  # (the ping-pong tile is one candidate per list: always kept)
                for ws in (WS if not thin else (WS[(i + M) % 3],)):
                    yield (f"slabs {M} {N} {K} {int(fp8)} {int(glu)} {nt:#x} {s} {ws}",
                           lib.gemm_partial_slabs(M, N, K, fp8, glu, 0, nt, s, ws))
                for kind in ((0, 1, 3) if not thin else ((0, 1, 3)[i % 3],)):
                    lib.gemm_tuned_clear()
                    lib.gemm_tuned_set(M, N, K, False, kind, nt, s)
                    got = (lib.gemm_plan(M, N, K, kind == 1), lib.gemm_tuned_get(M, N, K, False, kind),
                           lib.gemm_partial_slabs(M, N, K, kind == 1, False, 0, 0, 0, WS[0]))
                    yield f"plan {M} {N} {K} {kind} {nt:#x} {s}", got
                lib.gemm_tuned_clear()
            for tile in range(16):
                for sp in F8_SPLITS:
                    if thin and (tile + sp + M + N) % 7:
                        continue
                    for ws in (WS if not thin else (WS[(tile + sp) % 3],)):
                        yield (f"f8slabs {M} {N} {K} {int(glu)} {tile} {sp} {ws}",
                               lib.gemm_f8f8_partial_slabs(M, N, K, glu, 0, tile, sp, ws))


def replay(lib, key):
    """The value of one row, computed from its key alone (the committed sample outlives the candidate lists)."""
    kind, *f = key.split()
    if kind == "slabs":
        M, N, K, fp8, glu, nt, s, ws = (int(v, 0) for v in f)
        return lib.gemm_partial_slabs(M, N, K, bool(fp8), bool(glu), 0, nt, s, ws)
    if kind == "f8slabs":
        M, N, K, glu, tile, sp, ws = (int(v, 0) for v in f)
        return lib.gemm_f8f8_partial_slabs(M, N, K, bool(glu), 0, tile, sp, ws)
    M, N, K, tk, nt, s = (int(v, 0) for v in f)
    lib.gemm_tuned_clear()
    lib.gemm_tuned_set(M, N, K, False, tk, nt, s)
    try:
        return (lib.gemm_plan(M, N, K, tk == 1), lib.gemm_tuned_get(M, N, K, False, tk),
                lib.gemm_partial_slabs(M, N, K, tk == 1, False, 0, 0, 0, WS[0]))
    finally:
        lib.gemm_tuned_clear()


def lists(A):
    for M in MS:
        for N, K, glu, fp8 in SHAPES:
            yield f"candidates {M} {N} {K} {int(glu)} {int(fp8)}", A.candidates(M, N, K, glu, fp8)
            for neox in (False, True):
                yield f"qkv_epi_candidates {M} {N} {K} 128 {int(neox)}", A.qkv_epi_candidates(M, N, K, 128, neox)


def main(argv):
    import llmss_amd._C as lib
    from llmss_amd.ops import autotune as A

    thin = "--thin" in argv
    n = 0
    with open(argv[0], "w") as f:
        for k, v in rows(lib, A, thin):
            f.write(f"{k} = {v}\n")
            n += 1
        if not thin:
            for k, v in lists(A):
                f.write(f"{k} = {v}\n")
    print(n, "rows")


if __name__ == "__main__":
    main(sys.argv[1:])
