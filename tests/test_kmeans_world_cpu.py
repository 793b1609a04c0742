"""The conditions tests/test_gpu_kmeans_matrix.py rests on, on the reference alone (tests/kmeans_ref.py) and without a GPU: at
every dim, on ``oracle.normalize_c`` bits and the row count of 256 CUs, the emulated scores hold at least 50 exact-tie rows at
every nlist >= 21, every duplicate group wins rows (for its lowest list), every planted row goes to its own centroid, and at
nlist 200 every centroid that is neither a copy nor all zero wins a row.  The GPU file asserts the same on the bits the
index and the centroid packing actually store."""
import os
import re

import numpy as np
import pytest

import kmeans_ref as KR

CUS = 256


def test_shape_of_the_world():
    n = KR.n_rows(CUS)
    assert n == 17_541 and n % 32 == 5 and (-(-n // 16) * 16) % 32 == 16        # capacity pad16(n): half a block outside the slab
    total = -(-n // 32)
    assert total == 2 * CUS + 37                                                 # workgroups walk 2 or 3 row blocks
    assert KR.SPLIT % 16 not in (0,) and KR.SPLIT < n
    assert [KR.n_centroid_tiles(l) for l in KR.NLISTS] == [1, 1, 1, 1, 2, 2, 3, 3, 4, 7]
    assert {-(-KR.n_centroid_tiles(l) // 2) % 2 for l in KR.NLISTS} == {0, 1}    # both parities of the LDS buffer pair
    assert [-(-d // 128) * 128 for d in KR.DIMS] == [128, 256, 384, 512, 640, 768, 896, 1024]
    assert [d % 4 for d in (101, 498, 703)] == [1, 2, 3]
    ranges = KR.block_ranges(total)
    assert ranges == [(0, 1, 549), (0, 3, 183), (2, 3, 183), (5, 1, 544)]
    for first, step, nb in ranges:
        rows = KR.range_rows(first, step, nb)
        assert rows[(nb - 1) * 32] < n and (first + nb * step) * 32 >= n         # the range ends where the index does
    assert KR.range_rows(2, 3, 183)[-32] == 548 * 32                             # ... (2, 3) on the ragged last block
    dead = KR.dead_rows(CUS)
    assert len(set(dead.tolist())) == KR.N_DEAD and dead[0] == 0 and dead[-1] == n - 1


@pytest.mark.parametrize("dim", KR.DIMS)
def test_reference_conditions(oracle, dim):
    x, cent, owner, special = KR.make_world(dim, CUS)
    xb, cb = oracle.normalize_c(x), oracle.normalize_c(cent)
    for grp in KR.DUP_GROUPS:
        for j in grp[1:]:
            assert np.array_equal(cb[j].view(np.uint32), cb[grp[0]].view(np.uint32))
    assert not cb[KR.ZERO_CENTROID].any() and not xb[special["zero"]].any()
    ties = KR.check_world(KR.emulated(oracle, cb, xb), owner, special)
    print(f"dim {dim}: exact-tie rows per nlist {ties}")


def test_lds_buffer_parity_is_carried_across_row_blocks():
    """``pair``, the parity of the assign kernel's LDS double buffer, is deliberately NOT reset between the row blocks a
    persistent workgroup walks: the last tile pair of a block is ranked out of buffers ``pair ^ 2`` with no barrier behind it,
    so the next block's first dump must go to the other two.  Resetting it opens a race between a workgroup's fastest and
    slowest wave that no input can force (a build with ``pair = 0`` inside the loop passes the whole GPU matrix), so the
    source is held to it here: one initialisation in front of the row-block loop, one toggle behind the barrier."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "rassengine_amd", "csrc", "kmeans.hip")).read()
    body = src[src.index("void kmeans_assign_f32_kernel"):src.index("static hipError_t launch_assign_ch")]
    assert body.index("int pair = 0;") < body.index("for (int b = blockIdx.x")
    assert re.findall(r"\bpair\s*(?:[\^|&+*/%-]|<<|>>)?=(?!=)[^;]*;", body) == ["pair = 0;", "pair ^= 2;"]
    assert body.index("__syncthreads();") < body.index("pair ^= 2;") < body.rindex("rank_tile(Pa, pair ^ 2);")
