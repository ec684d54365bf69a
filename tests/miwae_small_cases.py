"""The edge shapes of the small-batch MIWAE step (csrc/vpc_miw_small.hip), shared by tests/test_miwae_small_gpu.py (GPU)
and tests/test_miwae_small_cases.py (CPU): whole-model cases of tests/miwae_cases.model_case at seed 0.

The kernels tile 16 decoder rows, give a workgroup RB = 1, 2 or 4 data rows of the stacked passes with all S samples of
each, and hold d <= 32 and L <= 16 as one or two 16-column tiles."""
import miwae_cases as C

SEED = 0
EDGE_SHAPES = [            # (B, S, d, L)
    (5, 20, 12, 10),       # B not a multiple of any RB, S = 20
    (17, 3, 32, 16),       # both width limits, a second encoder tile with one live row
    (7, 16, 13, 10),       # d % 4 != 0, S exactly one tile
    (2, 33, 12, 10),       # three tiles per row, the last with one live row
    (16, 16, 4, 2),        # every tile full
    (21, 20, 8, 10),       # empty rows on both passes (see edge_case)
]
EMPTY_ROWS_SHAPE = (21, 20, 8, 10)


def edge_case(shape, kind):
    """model_case(*shape, seed 0); at EMPTY_ROWS_SHAPE mask[3] = 0 and, for Reg_MIWAE, mask_p[3] = mask_p[7] = 0.  The
    cached arrays of model_case are left as they are: the changed masks are copies."""
    c = dict(C.model_case(*shape, kind == "reg", SEED))
    if shape == EMPTY_ROWS_SHAPE:
        m = c["mask"].copy()
        m[3] = 0
        c["mask"] = m
        if c["reg"]:
            mp = c["mask_p"].copy()
            mp[3] = 0
            mp[7] = 0
            c["mask_p"] = mp
    return c
