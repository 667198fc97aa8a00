"""The arithmetic of the workspace plan (csrc/plan.h: slots per chunk, the fit into an arena whose growth stopped short, rank head-room) with no GPU.
tests/host/plan_check.cpp is built against the header with the address and undefined-behaviour sanitizers and run as a child process: cases go in
on standard input, one line of integers per case comes back, and this file compares.  Nothing is loaded into Python.  The expected values of the
tables are derived by hand from the rules as ensure_workspace had them (docs/history/workspace_unit.md); those of a posterior query's chunks and
blocks (query_chunk, query_block_cols) from the expressions the query units had (docs/history/query_stages.md)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, 'poisson-gpfa_amd', 'csrc')
SOURCE = os.path.join(ROOT, 'tests', 'host', 'plan_check.cpp')
MIB64 = 64 << 20


@pytest.fixture(scope='module')
def ask(tmp_path_factory):
    """ask(lines) -> the program's answers, a list of ints (floats where it prints one) per case"""
    gxx = shutil.which('g++')
    if gxx is None:
        pytest.skip('no g++ on this machine: the plan arithmetic is checked by a compiled host program')
    exe = str(tmp_path_factory.mktemp('plan_check') / 'plan_check')
    # (the sanitizers' runtimes linked into the program: it runs as it is wherever the suite runs, whatever else the loader brings along)
    r = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-static-libasan', '-static-libubsan',
                        '-I', CSRC, '-o', exe, SOURCE], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(lines):
        r = subprocess.run([exe], input=''.join(l + '\n' for l in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == '', (r.returncode, r.stderr[-2000:])
        out = [[float(v) if '.' in v or 'e' in v else int(v) for v in l.split()] for l in r.stdout.splitlines()]
        assert len(out) == len(lines)
        return out
    return run


# ---- slots per chunk ----------------------------------------------------------------------------------------------------------------------------
AMPLE = 10 ** 6                       # budget / per far above every target: chunk_trials alone binds
SLOT_TABLE = [(100, 0, 100, 0), (100, 100, 100, 0), (100, 48, 40, 1), (100, 20, 16, 1), (100, 12, 12, 1), (100, 1, 1, 1),
              (130, 64, 48, 1), (130, 33, 32, 1)]       # target, chunk_trials, B, B_capped


def test_slot_count_with_memory_ample(ask):
    got = ask(['slots %d %d %d' % (AMPLE, opt, target) for target, opt, _, _ in SLOT_TABLE])
    print(got)
    assert got == [[B, capped] for _, _, B, capped in SLOT_TABLE]


def test_slot_count_memory_bound(ask):
    # 57 -> 56, three chunks of 128, ceil(43 / 8) * 8 = 48
    assert ask(['slots 57 0 128']) == [[48, 1]]


def test_budget_below_one_slot(ask):
    B, capped = ask(['slots 0 0 100'])[0]                          # budget < per: budget / per = 0
    assert B < 1 and capped == 1


GRID_TARGETS = [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 130, 255, 256, 257, 300, 511, 512, 513, 599, 600]
GRID_FITS = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 57, 63, 64, 65, 100, 127, 128, 129, 200, 256, 257, 400, 511, 512, 600, 699, 700]
GRID_OPTS = [0, 1, 12, 20, 48, 64]


def test_slot_count_invariants(ask):
    cases = [(t, f, o) for t in GRID_TARGETS for f in GRID_FITS for o in GRID_OPTS]
    got = ask(['slots %d %d %d' % (f, o, t) for t, f, o in cases])
    print('%d cases' % len(cases))
    assert len(cases) >= 3000
    for (t, f, o), (B, capped) in zip(cases, got):
        bound = min(f, o) if o else f
        assert 1 <= B <= min(t, f), (t, f, o, B)
        assert not o or B <= o, (t, f, o, B)
        if not o and 16 <= f < t:
            assert B % 8 == 0, (t, f, o, B)
        assert capped == int(bound < t), (t, f, o, B, capped)


# ---- the fit after a growth that stopped short -----------------------------------------------------------------------------------------------------
def fit_case(B_full, floor, cap, target=None, b0=1000, b1=100, step_at=10 ** 6, step=0):
    def bytes_for(n):
        return b0 + b1 * n + (step if n >= step_at else 0)
    return 'fit %d %d %d %d %d %d %d %d %d %d' % (bytes_for(B_full), bytes_for(floor), cap, B_full, floor, B_full if target is None else target, b0, b1,
                                                  step_at, step), bytes_for


def test_fit_linear_measurement(ask):
    # bytes(n) = 1000 + 100 n.  128 slots: must 7400, need 13800, 10000 mapped: 64 + 2600 / 100 = 90 -> 88, two chunks -> 64.
    # 256 slots: need 26600, 20000 mapped: 64 + 12600 / 100 = 190 -> 184, two chunks -> 128 (13800 bytes).
    lines = [fit_case(128, 64, 10000)[0], fit_case(256, 64, 20000)[0]]
    assert lines[0] == 'fit 13800 7400 10000 128 64 128 1000 100 1000000 0' and lines[1].startswith('fit 26600 7400 20000 256 64 256 ')
    assert ask(lines) == [[64, 7400, 1, 0], [128, 13800, 1, 0]]


def test_fit_walks_down_a_step_in_the_measurement(ask):
    # + 5000 bytes from 100 slots on: need(256) = 31600, must = 7400, 16000 mapped.  The interpolation's slope is (31600 - 7400) / 192 = 126.04, so the
    # first guess is 64 + 8600 / 126.04 = 132 -> 128 (two chunks of 128 stay 128), which measures 18800 > 16000; the walk goes down by 8 through
    # 120, 112, 104 (16400) to 96, the first below the step: 10600 bytes.  2 * 96 < 256: not capped.  (The expressions as they stood inside ensure_workspace give the same: docs/history/workspace_unit.md.)
    line, bytes_for = fit_case(256, 64, 16000, step_at=100, step=5000)
    B, need, capped, short = ask([line])[0]
    print(B, need, capped, short)
    assert bytes_for(128) > 16000 and bytes_for(104) > 16000
    assert (B, need, capped, short) == (96, 10600, 0, 0)


def test_fit_short_of_its_floor(ask):
    # the floor itself measures more than is mapped: floor_slots come back, flagged (the caller's "workspace arena short of its floor")
    line, bytes_for = fit_case(128, 64, 7400, step_at=64, step=1)
    assert ask([line])[0] == [64, bytes_for(64), 1, 1]


def test_fit_invariants(ask):
    cases = []
    for B_full in (9, 16, 17, 64, 100, 128, 130, 256, 300, 513, 600):
        for floor in sorted({min(B_full, f) for f in (8, 13, 64, 128)}):
            for target in sorted({B_full, B_full + 1, 2 * B_full + 3, 600}):
                if target < B_full:
                    continue
                for step_at, step in ((10 ** 6, 0), (B_full // 2, 5000), (floor + 1, 700)):
                    line, bytes_for = fit_case(B_full, floor, 0, target=target, step_at=step_at, step=step)
                    need, must = bytes_for(B_full), bytes_for(floor)
                    for cap in sorted({must, must + 1, must + 99, (must + need) // 2, need - 1}):
                        if must <= cap < need:                      # (what arena_grow leaves behind when its budget runs out)
                            cases.append((fit_case(B_full, floor, cap, target=target, step_at=step_at, step=step)[0], bytes_for, B_full, floor, target, cap))
    got = ask([c[0] for c in cases])
    print('%d cases' % len(cases))
    assert len(cases) >= 1000
    walked = 0
    for (line, bytes_for, B_full, floor, target, cap), (B, need, capped, short) in zip(cases, got):
        assert B == floor or B % 8 == 0, line
        assert floor <= B <= B_full, line
        assert need == bytes_for(B), line
        assert need <= cap or B == floor, line
        assert short == int(need > cap) and capped == int(2 * B >= target), line
        walked += need <= cap and B + 8 <= B_full and bytes_for(B + 8) > cap
    assert walked > 0


# ---- chunks and blocks of a posterior query (csrc/query.h) --------------------------------------------------------------------------------------------
STAGE = 256 << 20                     # QUERY_STAGE_BYTES
ANY_BYTES = (0, 1, 181760, 10 ** 12)  # where the option decides, the bytes do not
QCHUNK_TABLE = [((100, 0, 0, 0), 100), ((100, 0, 26843545, 0), 10), ((100, 0, 300000000, 0), 1), ((100, 0, 0, 40), 40), ((100, 64, 0, 40), 40)] + \
               [((100, 7, b, 0), 7) for b in ANY_BYTES]            # (n, option, bytes per trial, cap) -> trials per chunk
# covat, low-rank, p = 10, T16 = 176, rpad = 256: (10 * 176 + 2 * 256) = 2272 staged rows x 10 latents x 8 bytes = 181760 per query time, 184 fit an
# eighth of the staging -> 176; pfunc at the same shape: (2 * 1760 + 512) = 4032 rows x 8 bytes = 32256 per functional, 1040 fit
QBLOCK_TABLE = [((0, 512, 181760), 176), ((0, 2048, 32256), 1040), ((0, 512, 4000000), 16), ((0, 48, 8), 48)] + \
               [((24, 512, b), 32) for b in ANY_BYTES[1:]] + [((24, 16, b), 16) for b in ANY_BYTES[1:]]     # (option, padded width, bytes per column) -> columns


def test_query_chunk_table(ask):
    got = ask(['qchunk %d %d %d %d %d' % (case + (STAGE,)) for case, _ in QCHUNK_TABLE])
    print(got)
    assert got == [[want] for _, want in QCHUNK_TABLE]


def test_query_block_cols_table(ask):
    got = ask(['qblock %d %d %d %d' % (case + (STAGE,)) for case, _ in QBLOCK_TABLE])
    print(got)
    assert got == [[want] for _, want in QBLOCK_TABLE]


# ---- rank head-room ------------------------------------------------------------------------------------------------------------------------------------
DIMS = (5120, 5120, 5000, 1024, 512, 500, 10)       # ld npad n rpad Tp T p: a 10-latent, 500-bin system at a fifth of full rank
DIMS_S = '%d %d %d %d %d %d %d' % DIMS
TARGET = 128


def scaled(slab, mt, dense, hh):
    return max(slab, min(dense, int(slab * hh) // 1024 * 1024)), max(mt, min(dense, int(mt * hh * hh) // 1024 * 1024))


@pytest.fixture(scope='module')
def sizes(ask):
    """base slabs, the dense slab, the bytes of the whole list at each head-room factor, the shared bytes"""
    slab, mt, dense = ask(['base %s 1' % DIMS_S])[0]
    ld, _, _, rpad, Tp, T, _ = DIMS
    yt = ld * rpad
    want = max(yt + max(Tp * rpad + T * T, yt // 2 + 64), rpad * rpad)
    assert (slab, mt, dense) == ((want + 1023) // 1024 * 1024, rpad * rpad, ld * ld)
    factors = (2.0, 1.75, 1.5, 1.25, 1.1, 1.0)
    got = ask(['bytes %s %d %d' % ((DIMS_S,) + scaled(slab, mt, dense, hh)) for hh in factors])
    return slab, mt, dense, {hh: per * TARGET for hh, (per, _) in zip(factors, got)}, got[0][1]


def test_headroom_first_plan_takes_the_full_factor(ask, sizes):
    slab, mt, dense, _, _ = sizes
    pick, s, m = ask(['headroom %s 2.0 0 %d %d' % (DIMS_S, 10 ** 13, TARGET)])[0]
    assert pick == 2.0
    assert (s, m) == (min(dense, 2 * slab) // 1024 * 1024, min(dense, 4 * mt) // 1024 * 1024) and s > slab and m > mt
    # the dense slab caps both: a rank near n
    d = '1024 1024 1000 640 128 100 10'
    b_slab, b_mt, b_dense = ask(['base %s 1' % d])[0]
    assert b_slab < b_dense < 2 * b_slab and b_mt < b_dense < 4 * b_mt
    assert ask(['headroom %s 2.0 0 %d %d' % (d, 10 ** 13, TARGET)])[0] == [2.0, b_dense, b_dense]


def test_headroom_replan_takes_what_the_mapped_bytes_hold(ask, sizes):
    slab, mt, dense, list_bytes, shared = sizes
    assert list_bytes[1.75] > list_bytes[1.5] > list_bytes[1.25] > list_bytes[1.1] > list_bytes[1.0]
    cap = shared + MIB64 + list_bytes[1.5]                      # 1.5 fits to the byte, 1.75 does not
    assert ask(['headroom %s 2.0 %d %d %d' % (DIMS_S, cap, 10 ** 13, TARGET)])[0] == [1.5] + list(scaled(slab, mt, dense, 1.5))
    assert ask(['headroom %s 2.0 %d %d %d' % (DIMS_S, cap - 1, 10 ** 13, TARGET)])[0] == [1.25] + list(scaled(slab, mt, dense, 1.25))
    # the option's factor bounds the candidates
    assert ask(['headroom %s 1.25 %d %d %d' % (DIMS_S, cap, 10 ** 13, TARGET)])[0] == [1.25] + list(scaled(slab, mt, dense, 1.25))


def test_headroom_replan_that_fits_no_candidate(ask, sizes):
    slab, mt, dense, list_bytes, shared = sizes
    cap = shared + MIB64 + list_bytes[1.1] - 1                  # not even 1.1 fits what is mapped: min(h, 1.25), to be grown for
    assert ask(['headroom %s 2.0 %d %d %d' % (DIMS_S, cap, list_bytes[1.25], TARGET)])[0] == [1.25] + list(scaled(slab, mt, dense, 1.25))
    assert ask(['headroom %s 1.2 %d %d %d' % (DIMS_S, cap, 10 ** 13, TARGET)])[0] == [1.2] + list(scaled(slab, mt, dense, 1.2))
    # ... and the unscaled sizes when even that exceeds the budget
    assert ask(['headroom %s 2.0 %d %d %d' % (DIMS_S, cap, list_bytes[1.25] - 1, TARGET)])[0] == [1.25, slab, mt]
    assert ask(['headroom %s 2.0 1 %d %d' % (DIMS_S, list_bytes[1.25] - 1, TARGET)])[0] == [1.25, slab, mt]
