"""CPU restatement of the chunk-cell-major pair-row ids (calls of >= 3 views, View::pairchunks): the sort kernel's
formula (binning.hip::cell_lists_from_masks - prefix over the 64-record chunks of a tile list, prefix over the cells of
a chunk, rank inside the cell) and the pair reduction's (render_bwd.hip::hgs_k_pair_reduce_ch - ballots over the masks of
a chunk's records, cell after cell) must name the same row for every (entry, cell) pair, the rows must tile [0, pairs)
and a cell's rows inside a chunk must be consecutive in list order (what makes both kernels stream).

The packed formats themselves - the tag word of a record, entpair.x - are not restated here alone: csrc/entryrec.h, the
header the kernels compile, is built for the host (tests/entryrec_host.cpp) and both id computations below encode and decode
through it; the Python `rec_tag` stays as an independent restatement that is compared with the C function."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class EntryRec:
    """csrc/entryrec.h compiled for the host: array entry points over the tag and entpair.x functions"""

    def __init__(self, so):
        self.L = ctypes.CDLL(so)
        for name, nargs in (("hgs_rec_tag_host", 5), ("hgs_tag_fields_host", 2), ("hgs_entpair_x_host", 3),
                            ("hgs_entpair_entry_host", 2), ("hgs_entpair_pairs_host", 2)):
            getattr(self.L, name).argtypes = [ctypes.c_int] + [ctypes.c_void_p] * nargs
            getattr(self.L, name).restype = None

    def _call(self, name, out_shape, *arrays):
        n = len(np.atleast_1d(arrays[0]))
        ins = [np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.uint32), (n,))) for a in arrays]
        out = np.zeros(out_shape(n), dtype=np.uint32)
        getattr(self.L, name)(n, *[a.ctypes.data for a in ins], out.ctypes.data)
        return out

    def rec_tag(self, mask, k, n, chunk_rows):
        """hgs_rec_tag over arrays (mask gives the length; k, n, chunk_rows broadcast)"""
        return self._call("hgs_rec_tag_host", lambda m: m, np.atleast_1d(mask), k, n, np.asarray(chunk_rows, dtype=np.uint32))

    def tag_fields(self, tags):
        """columns: hgs_tag_mask, hgs_tag_pos, hgs_tag_count, hgs_tag_chunk_rows"""
        return self._call("hgs_tag_fields_host", lambda m: (m, 4), np.atleast_1d(tags))

    def entpair_x(self, entry, pairs):
        return self._call("hgs_entpair_x_host", lambda m: m, np.atleast_1d(entry), pairs)

    def entpair_entry(self, x):
        return self._call("hgs_entpair_entry_host", lambda m: m, np.atleast_1d(x))

    def entpair_pairs(self, x):
        return self._call("hgs_entpair_pairs_host", lambda m: m, np.atleast_1d(x))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("entryrec") / "entryrec_host.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas",
                           os.path.join(ROOT, "tests", "entryrec_host.cpp"), "-o", so])
    return EntryRec(so)


def rec_tag(mask, k, n, chunk_rows):
    """entryrec.h::hgs_rec_tag, restated"""
    left = n - (k & ~63)
    return (mask & 0xffff) | ((k & 63) << 16) | ((min(left, 64) - 1) << 22) | ((1 << 28) if chunk_rows else 0)


def sort_ids(lib, masks, pair_base=0):
    """row id of (list position k, cell c) as the sort kernel computes it, and what it leaves per record: the tag word
    (the C hgs_rec_tag) and entpair.y"""
    n = len(masks)
    tags = lib.rec_tag(masks, np.arange(n), n, True)
    ids = {}
    chunk_pairs = [sum(bin(int(m)).count("1") for m in masks[c0:c0 + 64]) for c0 in range(0, n, 64)]
    chunk_first = np.concatenate([[0], np.cumsum(chunk_pairs)])            # S.tab[ch][16]: exclusive prefix over the chunks
    for ch, c0 in enumerate(range(0, n, 64)):
        chunk = masks[c0:c0 + 64]
        cp = 0
        for c in range(16):
            ex = 0                                                        # lanes before this one with bit c
            for lane, m in enumerate(chunk):
                if (int(m) >> c) & 1:
                    ids[(c0 + lane, c)] = pair_base + int(chunk_first[ch]) + cp + ex
                    ex += 1
            cp += ex                                                      # tot[c]: records of the chunk that reach cell c
    entpair_y = [pair_base + int(chunk_first[k // 64]) for k in range(n)]     # what the sort leaves per record: its chunk's first row
    return ids, int(chunk_first[-1]), entpair_y, tags


def reduce_ids(lib, tags, entpair_y):
    """the same ids as the reduction finds them from what the sort left per record (tag word, entpair.y), decoded by
    the C accessors: a wave per window of 64 records takes the chunks that START in it"""
    n = len(tags)
    f = lib.tag_fields(tags)
    tmask, tpos, tcount, trows = (f[:, j].tolist() for j in range(4))
    ids = {}
    handled = set()
    for w0 in range(0, n, 64):
        starts = [p for p in range(w0, min(n, w0 + 64)) if tpos[p] == 0]
        for p0 in starts:
            C = tcount[p0]
            assert trows[p0]
            cp = 0
            for c in range(16):
                rank = 0
                for l in range(C):
                    assert p0 + l not in handled or c > 0
                    if (tmask[p0 + l] >> c) & 1:
                        ids[(p0 + l, c)] = entpair_y[p0 + l] + cp + rank
                        rank += 1
                cp += rank
            handled.update(range(p0, p0 + C))
    assert handled == set(range(n))                                       # every record belongs to exactly one chunk
    return ids


def test_chunk_cell_major_ids_tile_the_rows_and_agree_between_sort_and_reduce(lib):
    rng = np.random.default_rng(5)
    for n in (1, 5, 63, 64, 65, 127, 128, 200, 437, 1000):
        for density in (0.05, 0.27, 0.9):
            masks = np.zeros(n, dtype=np.uint32)
            for c in range(16):
                masks |= (rng.random(n) < density).astype(np.uint32) << c
            if n > 3:
                masks[1] = 0                                              # an entry without pairs
                masks[2] = 0xffff                                         # one that reaches every cell
            a, pairs, ey, tags = sort_ids(lib, masks, pair_base=1000)
            assert tags.tolist() == [rec_tag(int(m), k, n, True) for k, m in enumerate(masks)]
            assert sorted(a.values()) == list(range(1000, 1000 + pairs))                       # a bijection onto the tile's rows
            b = reduce_ids(lib, tags, ey)
            assert a == b
            # the backward's side: consecutive list entries of a cell inside one chunk own consecutive rows
            for c in range(16):
                ks = [k for k in range(n) if (int(masks[k]) >> c) & 1]
                for k0, k1 in zip(ks, ks[1:]):
                    if k0 // 64 == k1 // 64:
                        assert a[(k1, c)] == a[(k0, c)] + 1
            # the reduction's side: the rows of an entry ascend with the cell (summation order = cell order)
            for k in range(n):
                rows = [a[(k, c)] for c in range(16) if (int(masks[k]) >> c) & 1]
                assert rows == sorted(rows)


def test_record_tag_fields(lib):
    for n in (1, 64, 65, 130, 4096):
        for k in (0, n // 2, n - 1):
            t = int(lib.rec_tag(0xbeef, k, n, True)[0])
            assert t & 0xffff == 0xbeef and (t >> 16) & 63 == k % 64 and (t >> 28) & 1 == 1
            assert ((t >> 22) & 63) + 1 == min(64, n - (k // 64) * 64)
            assert (int(lib.rec_tag(0, k, n, False)[0]) >> 28) & 1 == 0


def test_c_tag_equals_the_restatement_and_the_accessors_the_shifts(lib):
    rng = np.random.default_rng(11)
    masks = np.concatenate([np.array([0, 1, 0x8000, 0xffff, 0xbeef], dtype=np.uint32),
                            rng.integers(0, 1 << 16, size=64, dtype=np.uint32)])
    for n in (1, 63, 64, 65, 127, 130, 4096, 4097, 16384, 16385, 100000):
        ks = sorted({k for k in (0, 1, 62, 63, 64, 65, n // 2, n - 2, n - 1) if 0 <= k < n})
        assert 0 in ks and n - 1 in ks
        for k in ks:
            for chunk_rows in (False, True):
                tags = lib.rec_tag(masks, k, n, chunk_rows)
                want = [rec_tag(int(m), k, n, chunk_rows) for m in masks]
                assert tags.tolist() == want, (n, k, chunk_rows)
                f = lib.tag_fields(tags)
                assert f[:, 0].tolist() == [t & 0xffff for t in want]
                assert f[:, 1].tolist() == [(t >> 16) & 63 for t in want]
                assert f[:, 2].tolist() == [((t >> 22) & 63) + 1 for t in want]
                assert f[:, 3].tolist() == [(t >> 28) & 1 for t in want]
                # and what the fields mean: the mask, the place in the 64-record chunk, the chunk's records, the layout
                assert f[:, 0].tolist() == masks.tolist()
                assert set(f[:, 1].tolist()) == {k % 64} and set(f[:, 2].tolist()) == {min(64, n - (k // 64) * 64)}
                assert set(f[:, 3].tolist()) == {int(chunk_rows)}


def test_entpair_x_round_trip(lib):
    rng = np.random.default_rng(12)
    entries = np.concatenate([np.array([0, 1, 1 << 26, (1 << 27) - 1], dtype=np.uint32),
                              rng.integers(0, 1 << 27, size=1000, dtype=np.uint32)])
    for pairs in range(17):
        x = lib.entpair_x(entries, pairs)
        assert x.tolist() == [int(e) | (pairs << 27) for e in entries]
        assert lib.entpair_entry(x).tolist() == entries.tolist()
        assert lib.entpair_pairs(x).tolist() == [pairs] * len(entries)
