"""A generalized suffix array the oracle does not reach, verified on the device: 2^28 characters of DNA generated in HBM,
cut into reads of 100-150 characters, built by psacx_construct_gsa_dev_u32 and by 4 ranks (psacx_multi_construct_gsa_dev_u32)
and handed to psacx_check_gsa_dev_u32 / psacx_multi_check_gsa_dev_u32.  Both verdicts are zero; after two neighbouring SA
entries are exchanged on the device (ISA kept the inverse) the order counter must object.  gsac --check-device gives the
same verdicts from the command line."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1 << 28
HERE = os.path.dirname(os.path.abspath(__file__))


def read_offsets(n, seed=5):
    rng = np.random.RandomState(seed)
    off = np.concatenate([[0], np.cumsum(rng.randint(100, 151, size=n // 100 + 2))]).astype(np.uint64)
    return np.concatenate([off[off < n], [n]]).astype(np.uint64)


def swap_neighbours(lib, rctx, d_sa, d_isa_of, i_local):
    """SA[i], SA[i+1] of one block exchanged on the device, ISA (d_isa_of(position) -> (rank context, address)) fixed up."""
    two = np.empty(2, np.uint32)
    assert lib.psacx_copy_d2h(rctx, two.ctypes.data_as(C.c_void_p), C.c_void_p(d_sa + 4 * i_local), 8) == 0
    ranks = []
    for pos in two:
        c, addr = d_isa_of(int(pos))
        r = np.empty(1, np.uint32)
        assert lib.psacx_copy_d2h(c, r.ctypes.data_as(C.c_void_p), C.c_void_p(addr), 4) == 0
        ranks.append((c, addr, r))
    assert int(ranks[1][2][0]) == int(ranks[0][2][0]) + 1
    rev = np.ascontiguousarray(two[::-1])
    assert lib.psacx_copy_h2d(rctx, C.c_void_p(d_sa + 4 * i_local), rev.ctypes.data_as(C.c_void_p), 8) == 0
    for (c, addr, r), other in zip(ranks, (ranks[1][2], ranks[0][2])):
        assert lib.psacx_copy_h2d(c, C.c_void_p(addr), other.copy().ctypes.data_as(C.c_void_p), 4) == 0


def test_reads_beyond_the_oracle_one_gpu_and_four_ranks():
    import psac_amd
    from psac_amd._lib import PSACX_LCP
    off = read_offsets(N)
    m = off.size - 1
    vp = C.c_void_p
    ctx = psac_amd.Context(0)
    lib = ctx._lib
    held = []

    def alloc(nbytes):
        held.append(ctx.alloc(nbytes))
        return held[-1]
    try:
        d_text = alloc(N)
        ctx.check(lib.psacx_synth_text_dev(ctx.handle, vp(d_text), N, 0, 0, 17, 1024))
        d_off = alloc(off.nbytes); ctx.h2d(d_off, off)
        d_sa, d_isa, d_lcp = alloc(N * 4), alloc(N * 4), alloc(N * 4)
        ctx._pre()
        ctx.check(lib.psacx_construct_gsa_dev_u32(ctx.handle, vp(d_text), N, vp(d_off), m, 0, PSACX_LCP, vp(d_sa), vp(d_isa), vp(d_lcp)))
        assert psac_amd.check_gsa_device(ctx, d_text, N, d_off, m, d_sa, d_isa, d_lcp, 32) == [0, 0, 0, 0]
        assert psac_amd.check_gsa_device(ctx, d_text, N, d_off, m, d_sa, d_isa, None, 32) == [0, 0, 0, 0]
        # read as one text the same arrays are wrong: the plain checker is no judge of a string set
        plain = psac_amd.check_device(ctx, d_text, N, d_sa, d_isa, d_lcp, 32)
        assert plain[0] == 0 and plain[1] > 0
        swap_neighbours(lib, ctx.handle, d_sa, lambda pos: (ctx.handle, d_isa + 4 * pos), N // 2)
        err = psac_amd.check_gsa_device(ctx, d_text, N, d_off, m, d_sa, d_isa, d_lcp, 32)
        assert err[0] == 0 and err[1] > 0 and err[3] == 0, err
        ctx.check(lib.psacx_trim(ctx.handle))

        # the same reads on 4 ranks (sharing the device): blocks of the text are slices of d_text, the results fresh arrays
        mg = psac_amd.MultiContext([0] * 4)
        try:
            P = 4
            sizes = [N // P] * P
            offs = [r * (N // P) for r in range(P)]
            arr = lambda: [alloc(sizes[r] * 4) for r in range(P)]
            sa, isa, lcp = arr(), arr(), arr()
            vps, u64s = vp * P, C.c_uint64 * P
            mg._pre()
            mg.check(lib.psacx_multi_construct_gsa_dev_u32(mg.handle, vps(*[d_text + o for o in offs]), u64s(*sizes), off.ctypes.data_as(vp), m, 0, PSACX_LCP,
                                                           vps(*sa), vps(*isa), vps(*lcp)))
            text_blocks = [d_text + o for o in offs]
            assert mg.check_gsa_device(text_blocks, sizes, off, sa, isa, lcp, 32) == [0, 0, 0, 0]
            assert mg.check_gsa_device(text_blocks, sizes, off, sa, isa, None, 32) == [0, 0, 0, 0]
            swap_neighbours(lib, mg.rank_ctx(2), sa[2], lambda pos: (mg.rank_ctx(pos // sizes[0]), isa[pos // sizes[0]] + 4 * (pos % sizes[0])), sizes[2] // 3)
            err = mg.check_gsa_device(text_blocks, sizes, off, sa, isa, lcp, 32)
            assert err[0] == 0 and err[1] > 0 and err[3] == 0, err
        finally:
            mg.close()
    finally:
        for p in held:
            ctx.free(p)
        ctx.close()


def test_gsac_check_device(tmp_path):
    import subprocess
    gsac = os.path.join(os.path.dirname(HERE), "psac_amd", "bin", "gsac")
    assert os.path.exists(gsac), "gsac not built"
    rng = np.random.RandomState(2)
    read = bytes(rng.randint(65, 69, size=150).astype(np.uint8))
    strings = [bytes(rng.randint(65, 69, size=int(rng.randint(1, 200))).astype(np.uint8)) for _ in range(500)] + [read, read[:70], read] * 5
    f = tmp_path / "reads.txt"
    f.write_bytes(b"\n".join(strings) + b"\n")
    for extra in ([], ["--gpus-on-device", "0,3"]):
        for lcp in (["-l"], []):
            r = subprocess.run([gsac, "-f", str(f), "--check-device"] + lcp + extra, capture_output=True, text=True)
            assert r.returncode == 0 and "[SUCCESS] GSA correct" in r.stdout and "[ERROR]" not in r.stderr, r.stdout + r.stderr
    # -c and --check-device together: two verdicts
    r = subprocess.run([gsac, "-f", str(f), "-l", "-c", "--check-device"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("[SUCCESS] GSA correct") == 2, r.stdout + r.stderr
