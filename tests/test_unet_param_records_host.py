"""The fused UNet kernel's parameter-record tables as the host packer writes them (csrc/unet.hip, push_records; read on the device by
rec_load of csrc/unet_kernel.h): every field of every record of every conv holds, exactly, the float of the state dict -- conv bias,
GroupNorm weight and bias, the 1x1 residual conv's and the tail convs' biases -- or the inverse power-of-two scale restated here from the
weights, on a weight set whose every array carries a per-channel ramp of its own.  The packer runs on the host alone
(mmd_debug_unet_pack): no GPU."""
import numpy as np
import pytest

import unet_record_cases as R


@pytest.fixture(scope="module")
def packed():
    sd = R.ramped_state_dict()
    blob, tables = R.pack(sd)
    return sd, blob, tables, R.expected_fields(sd)


def test_ramps_leave_no_two_channels_and_no_two_arrays_alike():
    sd, s0 = R.ramped_state_dict(), R.synth.synth_unet_state_dict(0)
    assert list(sd) == list(s0) and len(sd) == 148
    factors = []
    for k in sd:
        assert sd[k].dtype == np.float32 and sd[k].shape == s0[k].shape and np.isfinite(sd[k]).all(), k
        axis = 1 if k.startswith("ups.") and k.endswith(".4.conv.weight") else 0
        other = tuple(a for a in range(sd[k].ndim) if a != axis)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.nanmedian(np.where(s0[k] != 0, sd[k] / s0[k], np.nan), axis=other) if other else sd[k] / s0[k]
        assert np.all(np.diff(f) > 0) and 0.44 < f[0] < f[-1] < 1.91, k       # a ramp: strictly rising over the output channels
        factors.append((round(float(f[0]), 4), round(float(f[-1]), 4)))
    assert len(set(factors)) == len(factors)                                   # ... and no two arrays share theirs


def test_directory_lists_every_conv_with_its_layout(packed):
    _, blob, tables, want = packed
    assert set(tables) == set(want) and len(tables) == 24 + 4 + 2
    spans = []
    for name, (kind, cpr, fields) in want.items():
        t = tables[name]
        C = fields[0].shape[0]
        assert (t.kind, t.channels, t.channels_per_record, t.n_fields) == (kind, C, cpr, len(fields)), name
        assert t.record_floats == (len(fields) * cpr + 3) // 4 * 4 and t.record_floats % 4 == 0, name
        assert (t.offset * 4) % 16 == 0, name                                  # 16-byte aligned (the block itself is 256-byte aligned)
        n = (C // cpr) * t.record_floats
        assert t.offset + n <= blob.size, name
        spans.append((t.offset, t.offset + n, name))
    spans.sort()
    for (_, hi, a), (lo, _, b) in zip(spans, spans[1:]):
        assert hi <= lo, (a, b)                                                # no two tables overlap
    # NT = 2 stages: {b0, b1, g0, g1, be0, be1, is0, is1}, 32 bytes; with the residual fields 48; ups.0 (NT = 1): {b, g, be, is}, 16 bytes,
    # {b, g, be, is, br, isr, 0, 0} 32
    assert [tables[k].record_floats for k in ("d01.a", "d00.a", "u01.a", "u00.a", "u01.b", "down0", "up0", "up1", "final", "final.out")] == \
        [8, 12, 4, 8, 4, 4, 4, 8, 8, 4]
    assert np.isfinite(blob).all()                                             # (the buffer was NaN before the packer filled it)


def test_every_field_of_every_record_is_the_source_float(packed):
    _, blob, tables, want = packed
    n_checked = 0
    for name, (_, cpr, fields) in want.items():
        t = tables[name]
        for f, src in enumerate(fields):
            got = R.read_field(blob, t, f)
            src = np.asarray(src, np.float32)
            assert got.shape == src.shape
            assert np.array_equal(got.view(np.uint32), src.view(np.uint32)), (name, f, np.flatnonzero(got != src)[:4])
            # the first and the last channel unit, spelled out as the lane addresses them
            for u in (0, t.channels // cpr - 1):
                rec = blob[t.offset + u * t.record_floats: t.offset + (u + 1) * t.record_floats]
                assert np.array_equal(rec[f * cpr:(f + 1) * cpr], src[u * cpr:(u + 1) * cpr]), (name, f, u)
            n_checked += src.size
        # the padding behind a record's fields is zero
        recs = blob[t.offset: t.offset + (t.channels // cpr) * t.record_floats].reshape(-1, t.record_floats)
        assert not recs[:, len(fields) * cpr:].any(), name
    assert n_checked == sum(f.size for _, _, fs in want.values() for f in fs) > 5000


def test_ups0_records_hold_one_channel_each(packed):
    """the NT = 1 layout: ups.0's wave owns channels 16 wave + lane % 16, one per lane -- record c is channel c"""
    sd, blob, tables, _ = packed
    t = tables["u00.a"]
    assert (t.channels, t.channels_per_record, t.record_floats, t.kind) == (64, 1, 8, R.EPI_RES)
    for c in (0, 1, 31, 63):
        rec = blob[t.offset + c * 8: t.offset + c * 8 + 8]
        assert rec[0] == sd["ups.0.0.blocks.0.block.0.bias"][c] and rec[1] == sd["ups.0.0.blocks.0.block.2.weight"][c]
        assert rec[2] == sd["ups.0.0.blocks.0.block.2.bias"][c] and rec[4] == sd["ups.0.0.residual_conv.bias"][c]
        assert rec[3] == R.inverse_scale(sd["ups.0.0.blocks.0.block.0.weight"], (1, 2))[c] and rec[6] == rec[7] == 0
    t = tables["up0"]
    for c in (0, 63):
        rec = blob[t.offset + c * 4: t.offset + c * 4 + 4]
        assert rec[0] == sd["ups.0.4.conv.bias"][c] and rec[3] == 0
        assert rec[1] == R.inverse_scale(sd["ups.0.4.conv.weight"][:, :, [3, 1]], (0, 2))[c]
        assert rec[2] == R.inverse_scale(sd["ups.0.4.conv.weight"][:, :, [2, 0]], (0, 2))[c]


def test_inverse_scales_are_powers_of_two_that_differ_across_channels(packed):
    """what makes a misplaced scale field visible: on the ramped weights every conv's inverse scales take more than one value"""
    _, blob, tables, want = packed
    for name, (kind, _, fields) in want.items():
        for f in {R.EPI: (3,), R.EPI_RES: (3, 5), R.TAIL_DOWN: (1,), R.TAIL_UP: (1, 2), R.OUT: (1,)}[kind]:
            got = R.read_field(blob, tables[name], f)
            m, _ = np.frexp(got)
            assert np.all(m == 0.5) and (len(np.unique(got)) > 1 or name == "final.out"), (name, f)


def test_size_query_and_refusals():
    import ctypes as C
    lib = R._lib.load()
    sd = R.ramped_state_dict()
    blob, tables = R.pack(sd)
    blob2, _ = R.pack(sd)
    assert np.array_equal(blob.view(np.uint32), blob2.view(np.uint32))         # deterministic
    assert blob.size % 4 == 0
    assert lib.mmd_debug_unet_pack(32, 4, 25, None, None, 0, None, 0, None, None, 0, None) != 0 and b"fused" in lib.mmd_last_error()
    assert "mmd_debug_unet_pack" in R._lib.DEBUG_SYMBOLS and C.sizeof(R.RecordTable) == 48
