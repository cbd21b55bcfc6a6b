"""The *_workspace_bytes functions of the forward sources (fwd_blocks.hip, pct.hip, scone_vis.hip, scone_occ.hip) and of the backward sources (bwd_blocks.hip, attention_bwd.hip, pct_bwd.hip,
scone_vis_bwd.hip, scone_occ_bwd.hip), one library against another (plain host code: no GPU).

    python tools/compare_workspace_sizes.py OLD/libmacarons_hip.so NEW/libmacarons_hip.so

For every entry and every size of a grid (the sizes bench.py --full times, small and odd ones): NEW may exceed OLD by at most 256 B per
carved region of the entry (each region is rounded up to 256 B; nothing else may grow), and where NEW is smaller the difference is
printed.  Exits 1 on a violation.
"""
import ctypes
import itertools
import sys

I64, CI = ctypes.c_int64, ctypes.c_int
BQ = [(1, 16), (1, 300), (1, 16385), (1, 100000), (8, 32768), (8, 4096), (3, 777), (30, 2048), (41, 2048), (2, 16384)]
SL = [(1, 16), (1, 2048), (8, 2048), (30, 2048), (41, 2048), (3, 333), (16, 256), (100000, 16), (16385, 16), (1, 10240)]
# entry -> (argument types, argument grid, regions carved)
ENTRIES = {
    "mcr_pc_transformer_workspace_bytes": ((I64, I64), SL, 4),
    "mcr_scone_vis_workspace_bytes": ((I64, I64), SL[:7] + [(1, 17)], 4),
    "mcr_scone_vis_backward_workspace_bytes": ((I64, I64), SL[:7] + [(1, 17)], 28),
    "mcr_scone_occ_workspace_bytes": ((I64, I64, I64), [(b, q, lg) for (b, q) in BQ for lg in (2048, 16, 1000)], 18),
    "mcr_scone_occ_ragged_workspace_bytes": ((I64, I64, I64), list(itertools.product((1, 8, 27, 30, 41, 64), (16, 1000, 16385, 40000, 100000),
                                                                                     (2048, 512))), 12),
    "mcr_attention_backward_workspace_bytes": ((I64, I64, CI, CI), [(s, l, 4, 256) for (s, l) in SL[:7] + [(2, 17)]], 4),
    "mcr_linear_backward_workspace_bytes": ((I64, CI, CI), [(m, n, k) for m in (1, 16, 777, 61440, 83968) for (n, k) in
                                                            ((126, 4), (384, 256), (512, 256), (256, 512), (64, 128), (7, 5))], 3),
    "mcr_layernorm_backward_workspace_bytes": ((I64, CI), [(m, e) for m in (1, 16, 4097, 61440, 83968) for e in (64, 128, 256, 512)], 1),
    "mcr_attention_backward_pct_workspace_bytes": ((I64, I64), SL + [(2, 17), (2, 2049), (65535, 16)], 4),
    # (S, L): L == 16 on both sides of the 2048-sequence chunk, long sequences with S on both sides of the attention's split
    "mcr_pc_transformer_backward_workspace_bytes": ((I64, I64), SL + [(2047, 16), (2048, 16), (2049, 16), (2, 2049), (3, 2047), (1, 17)], 24),
    # (B, Q, Lg, q_chunk): Q on both sides of the default chunk, q_chunk 0 (the default) and 16 and a larger one
    "mcr_scone_occ_backward_workspace_bytes": ((I64, I64, I64, I64), [(b, q, lg, qc) for (b, q) in ((1, 16), (1, 300), (2, 48), (1, 2047),
                                                                                                     (1, 2048), (3, 2049), (8, 4096), (41, 777))
                                                                    for lg in (2048, 16, 1000) for qc in (0, 16, 1024)], 63),
    # (J, T, Lg, q_chunk): one job and a few dozen, T on both sides of the default chunk
    "mcr_scone_occ_backward_ragged_workspace_bytes": ((I64, I64, I64, I64), list(itertools.product((1, 3, 27, 41), (16, 1000, 2047, 2049, 40000),
                                                                                                   (2048, 512, 17), (0, 16, 1024))), 63),
    "mcr_attention_planes_workspace_bytes": ((I64, I64, CI, CI, CI), [(s, l, 4, qk, v) for (s, l) in ((1, 2048), (30, 2048), (41, 2048), (2, 700),
                                                                                                     (3, 333), (1, 16)) for (qk, v) in ((32, 128), (64, 256))], 2),
}


def main(old_path, new_path):
    old, new = ctypes.CDLL(old_path), ctypes.CDLL(new_path)
    bad = 0
    for name, (types, grid, regions) in ENTRIES.items():
        f_old, f_new = getattr(old, name), getattr(new, name)
        f_old.restype = f_new.restype = ctypes.c_size_t
        grew, shrank, worst_up, worst_down = 0, 0, 0, 0
        for args in grid:
            a = [t(v) for t, v in zip(types, args)]
            o, n = f_old(*a), f_new(*a)
            if n > o:
                grew += 1
                worst_up = max(worst_up, n - o)
                if n - o > 256 * regions:
                    bad += 1
                    print(f"VIOLATION {name}{args}: {o} -> {n} (+{n - o} > 256 x {regions})")
            elif n < o:
                shrank += 1
                worst_down = max(worst_down, o - n)
        print(f"{name}: {len(grid)} sizes, {len(grid) - grew - shrank} equal, {grew} larger (at most +{worst_up} B; bound {256 * regions}), "
              f"{shrank} smaller (at most -{worst_down} B)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
