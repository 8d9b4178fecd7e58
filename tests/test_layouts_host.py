"""The Python side's definition of the four spike layouts (``spkdiff.ops``: LAYOUTS, ``layout_of``, ``empty_spikes``) on CPU
tensors: no GPU, no library call.  The shapes and dtypes are those of DESIGN.md §3."""
import pytest
import torch

from spkdiff import ops

B, C, H, W, T = 3, 64, 5, 7, 16


def test_the_table_lists_the_four_layouts():
    assert [l.name for l in ops.LAYOUTS] == ["PTC", "CPTC", "C4", "S32"]
    assert (ops.C4.dtype, ops.C4.rec_channels, ops.C4.rec_bytes, ops.C4.chunk) == (torch.int8, 64, 32, ops.CHUNK_C4)
    assert (ops.S32.dtype, ops.S32.rec_channels, ops.S32.rec_bytes, ops.S32.chunk) == (torch.int8, 32, 16, ops.CHUNK_S32)
    assert ops.PTC.dtype == torch.uint8 and ops.C4_DTYPE == torch.int8
    assert (ops.CHUNK_C4, ops.CHUNK_S32) == (-64, -32)                      # include/spkdiff.h SPK_CHUNK_C4 / SPK_CHUNK_S32
    c = ops.cptc(32)
    assert (c.name, c.dtype, c.rec_channels, c.rec_bytes, c.chunk) == ("CPTC", torch.uint8, 32, 32, 32) and ops.LAYOUTS[1] == c
    assert (ops.PTC.rec_channels, ops.PTC.rec_bytes, ops.PTC.chunk) == (0, 0, 0)      # 0: all C channels of the tensor
    with pytest.raises(AttributeError):
        ops.C4.rec_bytes = 16                                               # immutable


@pytest.mark.parametrize("shape,dtype,name,rec", [
    ((B, H, W, T, C), torch.uint8, "PTC", (0, 0)),
    ((B, C // 4, H, W, T, 4), torch.uint8, "CPTC", (4, 4)),
    ((B, C // 32, H, W, T, 32), torch.uint8, "CPTC", (32, 32)),             # against C4 of the same shape: 128 channels there
    ((B, C // 32, H, W, T, 32), torch.int8, "C4", (64, 32)),
    ((B, C // 16, H, W, T, 16), torch.uint8, "CPTC", (16, 16)),             # against S32 of the same shape
    ((B, C // 16, H, W, T, 16), torch.int8, "S32", (32, 16)),
    ((B, 1, H, W, 4, 16), torch.int8, "S32", (32, 16)),
])
def test_layout_of_names_the_layout_and_its_dimensions(shape, dtype, name, rec):
    lay, dims = ops.layout_of(torch.zeros(shape, dtype=dtype))
    assert lay.name == name and lay.dtype == dtype and (lay.rec_channels, lay.rec_bytes) == rec
    assert dims == (B, C if name == "PTC" else shape[1] * rec[0], H, W, shape[-2])
    assert all(type(v) is int for v in dims)
    assert lay == (ops.cptc(rec[0]) if name == "CPTC" else getattr(ops, name))


@pytest.mark.parametrize("t", [
    torch.zeros((B, H, W, C), dtype=torch.uint8),                           # 4-D
    torch.zeros((B, 2, H, W, T, 8), dtype=torch.int8),                      # int8 records of 8 bytes: neither C4 nor S32
    torch.zeros((B, H, W, T, C), dtype=torch.int8),                         # the int8 tag on a plain PTC shape
    torch.zeros((T, B, C, H, W), dtype=torch.float32),                      # the interface tensor is no stored layout
], ids=["4d", "int8-rec8", "int8-5d", "fp32"])
def test_layout_of_refuses_what_is_none_of_the_four(t):
    with pytest.raises((NotImplementedError, ValueError)):
        ops.layout_of(t)


@pytest.mark.parametrize("layout,channels,shape,dtype", [
    (ops.PTC, 64, (B, H, W, T, 64), torch.uint8),
    (ops.PTC, 3, (B, H, W, T, 3), torch.uint8),
    (ops.cptc(32), 64, (B, 2, H, W, T, 32), torch.uint8),
    (ops.cptc(4), 64, (B, 16, H, W, T, 4), torch.uint8),
    (ops.C4, 64, (B, 1, H, W, T, 32), torch.int8),
    (ops.C4, 128, (B, 2, H, W, T, 32), torch.int8),
    (ops.S32, 32, (B, 1, H, W, T, 16), torch.int8),
    (ops.S32, 64, (B, 2, H, W, T, 16), torch.int8),
    (ops.S32, 16, (B, 1, H, W, T, 16), torch.int8),                         # a partly filled record: ceil(C / 32)
    (ops.S32, 48, (B, 2, H, W, T, 16), torch.int8),
])
def test_empty_spikes_spells_the_record_shapes(layout, channels, shape, dtype):
    t = ops.empty_spikes(layout, B, channels, H, W, T, "cpu")
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    lay, dims = ops.layout_of(t)
    assert lay.name == layout.name
    rc = lay.rec_channels or channels
    assert dims == (B, -(-channels // rc) * rc, H, W, T)


def test_the_wrappers_refuse_cpu_tensors_before_anything_else():
    for fn in (ops.ptc_to_spikes, ops.c4_to_spikes, ops.s32_to_spikes, ops.count_spikes):
        with pytest.raises(RuntimeError):
            fn(torch.zeros((B, 1, H, W, T, 16), dtype=torch.int8))
