"""The device bundle loop's contract (csrc/host/fa_dl.h) through libfa_host.so's
fa_dl_layout export: Python holds no copy of it, so the table here is the oracle -- the
values gen.hip, levels.hip, count.hip and ops/primitives.py each used to write out."""
import ctypes

import numpy as np

# control block slots (slot 4 under both of its meanings), limits, slab mode bits
VALUES = dict(
    kDlStop=0, kDlLevels=1, kDlTotal=2, kDlLastC=3, kDlTmax=4, kDlOverBound=4, kDlMulti=5, kDlNUsed=6, kDlEnd=7,
    kDlNl=8, kDlCl=40, kDlGl=72, kDlEmpty=104, kDlPieces=220, kDlPiecesI32=221, kDlBits=512, kDlBitsW=512,
    kDlCtl=1024,
    kDlMaxM=40, kDlMaxLevels=31, kDlMaxL=32, kDlInline=12, kAgMaxF1=32768,
    kSlabCls=1, kSlabDense=2, kSlabAcc16=4,
    kSlabFlagDense=4, kSlabFlagAcc16=8, kSlabFlagPartShift=8, kSlabFlagNpartsShift=16, kSlabFlagPartMask=255)
DESC_FIELDS = ("P", "cnt", "off", "rows", "m", "n", "C", "base")


def test_every_exported_constant_has_its_value(native):
    from fastapriori_amd.ops import primitives as Pm
    K = Pm.dl()
    consts = {n: v for n, v in K.table.items() if n.isidentifier()}
    assert consts == VALUES
    assert all(getattr(K, n) == v for n, v in VALUES.items())
    # every other entry is a struct's size or a field's offset
    assert all(n.startswith(("sizeof(Dl", "DlDesc.", "DlPost.")) for n in K.table if n not in consts)


def test_dlpost_matches_the_native_struct(native):
    from fastapriori_amd.ops import primitives as Pm
    K = Pm.dl()
    assert ctypes.sizeof(Pm.DlPostC) == 264 == K.post_size
    fields = [n for n, _ in Pm.DlPostC._fields_]
    assert len(fields) == 33 and sorted(fields) == sorted(K.post_offsets)
    for n in fields:
        assert getattr(Pm.DlPostC, n).offset == K.post_offsets[n], n
        assert getattr(Pm.DlPostC, n).size == 8, n


def test_descriptor_dtype_is_dldesc(native):
    from fastapriori_amd.ops import primitives as Pm
    K = Pm.dl()
    dt = K.desc_dtype
    assert dt.itemsize == 64 == K.table["sizeof(DlDesc)"]
    assert dt.names == DESC_FIELDS
    for i, n in enumerate(DESC_FIELDS):
        assert dt.fields[n] == (np.dtype(np.int64), 8 * i), n
        assert K.table["DlDesc." + n] == 8 * i


def test_level_table_rows_by_name_and_by_position(native):
    from fastapriori_amd.ops import primitives as Pm
    K = Pm.dl()
    t = np.zeros(K.kDlMaxL, dtype=K.desc_dtype).view(Pm._DescTable)
    assert t.nbytes == 32 * 64
    t[3] = [10, 11, 12, 13, 14, 15, 16, 17]          # DlDesc's order
    assert [int(t[3][n]) for n in DESC_FIELDS] == list(range(10, 18))
    assert t.view(np.int64).reshape(32, 8)[3].tolist() == list(range(10, 18))
    t[3]["C"] = 5
    assert t["C"][:4].tolist() == [0, 0, 0, 5]
    t[:] = 0
    assert not t.view(np.int64).any()
