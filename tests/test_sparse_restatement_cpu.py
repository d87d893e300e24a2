"""tests/sparse_restate.py against a case written out by hand, and its round trip."""
import numpy as np

import sparse_restate as sr
from hydra_amd import synth


def test_hand_case():
    # M = 2, N = 5.  Marker 0: genotypes [2, 1, 0, missing, 1]: fields 00, 10, 11, 01 in byte 0 (low bits first), 10 in byte 1.
    # Marker 1: all 0: fields 11.  The slots of byte 1 beyond row 4 hold 00 here, which is genotype 2: they must not be read.
    bed = np.array([[0b01111000, 0b00000010],
                    [0b11111111, 0b00000011]], dtype=np.uint8)
    got = sr.bed_to_lists(bed, 5)
    want = {
        "sl1": [2, 0], "ss1": [0, 2], "si1": [1, 4],
        "sl2": [1, 0], "ss2": [0, 1], "si2": [0],
        "slm": [1, 0], "ssm": [0, 1], "sim": [3],
    }
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == (np.uint32 if k.startswith("si") else np.uint64), k
        assert got[k].tolist() == v, k
    files = sr.file_bytes(got, 5, 2)
    assert files["dim"] == b"5 2\n"
    assert files["ss1"] == (0).to_bytes(8, "little") + (2).to_bytes(8, "little")
    assert files["si1"] == (1).to_bytes(4, "little") + (4).to_bytes(4, "little")
    assert len(files) == 10
    # back: the same columns, the slots beyond N as the missing code
    back = sr.lists_to_bed(got, 5, 2)
    assert back.tolist() == [[0b01111000, 0b01010110], [0b11111111, 0b01010111]]
    # the library's own packer agrees with the literal bytes where rows exist
    assert synth.pack_bed_columns(np.array([[2, 1, 0, 3, 1], [0, 0, 0, 0, 0]], dtype=np.uint8)).tolist() == back.tolist()


def test_round_trip_with_missing_calls():
    for N in (1, 4, 5, 63, 130):
        geno = synth.make_genotypes(9, N, seed=N, missing_rate=0.1) if N > 1 else np.array([[1], [3], [0], [2]], dtype=np.uint8)
        M = geno.shape[0]
        bed = synth.pack_bed_columns(geno)
        lists = sr.bed_to_lists(bed, N)
        for c, g in zip(sr.CLASSES, (1, 2, 3)):
            assert lists["sl" + c].tolist() == (geno == g).sum(axis=1).tolist()
            for j in range(M):
                a = int(lists["ss" + c][j])
                assert lists["si" + c][a:a + int(lists["sl" + c][j])].tolist() == np.flatnonzero(geno[j] == g).tolist()
        assert np.array_equal(sr.lists_to_bed(lists, N, M), bed)
