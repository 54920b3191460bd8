"""GPU suite: device bit packing vs a restatement of the reference's BitPacker / BitUnpacker, and .ecdc round trips.

Truth is ref_bitpack / ref_bitunpack of tests/audio_judge.py: Python integers, independent of the kernels, held to a hand-worked answer in
tests/test_containers_cpu.py.  The op tests below the first one run every width from 1 to 24 bits at shapes whose rows end on every
possible bit of a byte, with the patterns that show a shift leaking into a neighbour, through the host-pointer forms and through the
device-pointer forms on canary-filled buffers (tests/audio_judge.py: Canvas) at the byte alignments the multi-GPU all-gather produces.
Each prints one `OPREPORT {...}` line (run with -s); NC_AUDIO_REPORT=<path> writes the table (see tests/test_audio_gpu.py).
"""
import io
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import audio_judge as J  # noqa: E402
from audio_judge import ref_bitpack, ref_bitunpack  # noqa: E402
from conftest import encodec_cfg_from_meta, load_golden  # noqa: E402
from neuralcodecs_amd import Encodec, _lib, containers  # noqa: E402
from neuralcodecs_amd.weights import encodec_synthetic_state_dict, save_blob, synthetic_pcm  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _write_table():
    yield
    J.write_table()


@pytest.mark.parametrize("bits,K,T,B", [(10, 8, 150, 2), (10, 9, 87, 3), (1, 3, 5, 1), (7, 4, 33, 2), (12, 4, 100, 1), (24, 2, 9, 2),
                                        (8, 8, 4, 1)])
def test_pack_unpack_matches_reference_bitpacker(bits, K, T, B):
    rng = np.random.default_rng(bits * 100 + K)
    codes = rng.integers(0, 1 << bits, (B, K, T), dtype=np.int64)
    packed = containers.pack_codes(codes, bits)
    for b in range(B):
        want = ref_bitpack(codes[b].T.reshape(-1), bits)                       # t outer, k inner (EncodecCompressor.cs:170-181)
        assert packed[b].tobytes() == want
        assert ref_bitunpack(packed[b].tobytes(), bits, K * T) == codes[b].T.reshape(-1).tolist()
    assert np.array_equal(containers.unpack_codes(packed, K, T, bits), codes)
    with pytest.raises(ValueError):
        containers.pack_codes(np.full((1, 1, 1), 1 << bits), bits)            # ArgumentOutOfRangeException
    with pytest.raises(EOFError):
        containers.unpack_codes(packed[:, :-1], K, T, bits)                   # "Stream ended too soon"


def test_ecdc_roundtrip_48k_style_with_tail():
    g = load_golden("encodec_small48")
    cfg = encodec_cfg_from_meta(g["meta"])
    m = Encodec(cfg)
    m.load_blob(save_blob(encodec_synthetic_state_dict(cfg, seed=g["meta"]["weight_seed"])))
    wav = g["pcm"][0]
    blob = containers.ecdc_compress(m, wav)
    # byte-level layout: header, then per frame BE (1, scale) + bit-packed codes
    meta = containers.ecdc_read_header(io.BytesIO(blob))
    assert (meta["m"], meta["al"], meta["nc"], meta["lm"], meta["ch"]) == ("encodec_16khz", 8100, 2, False, 2)
    frames = m.encode(wav[None])
    body = io.BytesIO(blob)
    containers.ecdc_read_header(body)
    for f in frames:
        assert struct.unpack(">i", body.read(4))[0] == 1
        assert struct.unpack(">f", body.read(4))[0] == np.float32(f.scale[0, 0])
        want = ref_bitpack(np.asarray(f.codes)[0].T.reshape(-1), m.bits_per_codebook)
        assert body.read(len(want)) == want
    assert body.read() == b""
    out, sr = containers.ecdc_decompress(m, blob)
    assert sr == cfg.sampling_rate and out.shape == wav.shape
    assert np.array_equal(out, m.decode(frames, wav.shape[-1])[0, :, : wav.shape[-1]])
    with pytest.raises(EOFError):
        containers.ecdc_decompress(m, blob[:-3])
    m.dispose()


# ============================================================================================ nc_pack.hip, one operation at a time
OK = _lib.NC_OK


def _pad_mask(n_values, bits):
    """The bits of a row's last byte that belong to no value."""
    used = (n_values * bits) % 8
    return 0 if used == 0 else (0xFF << used) & 0xFF


def _pack_dev(codes, bits, skew=0, stream=None):
    """nc_pack_codes_dev on canary-filled buffers; the packed rows start `skew` bytes behind a 16-byte boundary."""
    B, K, T = codes.shape
    nbytes = _lib.lib().nc_packed_bytes(K * T, bits)
    src, dst = J.Canvas(np.int64, codes.size, codes), J.Canvas(np.uint8, B * nbytes, skew=skew)
    assert dst.ptr % 16 == skew
    assert _lib.lib().nc_pack_codes_dev(0, src.ptr, B, K, T, bits, dst.ptr, stream) == OK
    return dst.read(f"pack bits={bits} skew={skew}").reshape(B, nbytes)


def _unpack_dev(packed, K, T, bits, skew=0, stream=None):
    B = packed.shape[0]
    src, dst = J.Canvas(np.uint8, packed.size, packed, skew=skew), J.Canvas(np.int64, B * K * T)
    assert src.ptr % 16 == skew
    assert _lib.lib().nc_unpack_codes_dev(0, src.ptr, B, K, T, bits, dst.ptr, stream) == OK
    return dst.read(f"unpack bits={bits} skew={skew}").reshape(B, K, T)


@pytest.mark.parametrize("bits", range(1, 25))
def test_every_width_packs_and_unpacks_as_the_reference_bitpacker(bits):
    """Every shape of J.PACK_SHAPES with 1 and 3 rows, random values and the bleed patterns: packed bytes equal the Python-integer
    packer (so the pad bits of a row's last byte are 0), and unpacking gives the codes back."""
    assert J.tail_residues(bits) == J.possible_residues(bits) and 0 in J.tail_residues(bits)
    compared, names = 0, set()
    for K, T in J.PACK_SHAPES:
        for B in J.PACK_ROWS:
            for name, stream in J.pack_patterns(bits, K, T, B):
                names.add(name)
                codes, want = J.to_codes(stream, K, T), J.ref_pack_rows(stream, bits)
                what = f"bits={bits} K={K} T={T} B={B} {name}"
                packed = containers.pack_codes(codes, bits)
                assert packed.shape == want.shape and packed.dtype == np.uint8, what
                assert np.array_equal(packed, want), f"{what}: packed bytes differ at {np.argwhere(packed != want)[:4].tolist()}"
                assert (packed[:, -1] & _pad_mask(K * T, bits) == 0).all(), what
                back = containers.unpack_codes(packed, K, T, bits)
                assert back.dtype == np.int64 and np.array_equal(back, codes), f"{what}: unpacked codes differ"
                assert ref_bitunpack(packed[-1].tobytes(), bits, K * T) == stream[-1].tolist()
                compared += int(packed.size + back.size)
    assert {"random", "ones", "alternating", "alternating-odd", "single-first", "single-last"} <= names
    assert ("single-three-bytes" in names) == (bits >= 10 and bits not in (10, 12, 16))
    J.report("pack+unpack", case=f"bits{bits}", patterns=sorted(names), compared=compared, mismatches=0)


@pytest.mark.parametrize("bits", range(1, 25))
def test_unpack_ignores_the_pad_bits_and_the_next_row(bits):
    """Three rows: the first byte of every row is 0xFF, the last values of every row are 0, and the pad bits of every row's last byte are
    set to 1 before unpacking.  A value that read past its own bits, or a row that read into the next, comes out non-zero."""
    compared = 0
    for K, T in J.PACK_SHAPES:
        n, full = K * T, (1 << bits) - 1
        stream = np.random.default_rng([bits, K, T]).integers(0, 1 << bits, (3, n), dtype=np.int64)
        stream[:, -(n // 2):] = 0
        stream[:, :min(n, -(-8 // bits))] = full
        packed = J.ref_pack_rows(stream, bits).copy()
        if n * bits >= 8:
            assert (packed[:, 0] == 0xFF).all()
        packed[:, -1] |= _pad_mask(n, bits)
        for got in (containers.unpack_codes(packed, K, T, bits), _unpack_dev(packed, K, T, bits, skew=1)):
            assert np.array_equal(got, J.to_codes(stream, K, T)), f"bits={bits} K={K} T={T}"
            compared += int(got.size)
    J.report("unpack", case=f"padding-bits{bits}", compared=compared, mismatches=0)


@pytest.mark.parametrize("skew", [0, 1, 3])
def test_device_pointer_forms_at_unaligned_rows_equal_the_host_pointer_forms(skew):
    """The all-gather of nc_group.hip packs into, and unpacks from, rows at any byte offset.  0xA5 on either side of the rows must
    survive, and the bytes equal those of nc_pack_codes / nc_unpack_codes."""
    import torch
    side = torch.cuda.Stream() if skew == 3 else None
    compared = 0
    for bits in (1, 3, 7, 8, 10, 11, 13, 16, 17, 23, 24):
        for K, T in ((9, 87), (3, 5), (1, 1), (32, 3)):
            stream = np.random.default_rng([bits, K, T, skew]).integers(0, 1 << bits, (3, K * T), dtype=np.int64)
            codes = J.to_codes(stream, K, T)
            host = containers.pack_codes(codes, bits)
            assert np.array_equal(host, J.ref_pack_rows(stream, bits))
            s = side.cuda_stream if side is not None and bits == 11 else None     # once on a side stream
            packed = _pack_dev(codes, bits, skew, s)
            assert np.array_equal(packed, host), f"bits={bits} K={K} T={T}: device-pointer pack differs from the host-pointer form"
            back = _unpack_dev(host, K, T, bits, skew, s)
            assert np.array_equal(back, containers.unpack_codes(host, K, T, bits)) and np.array_equal(back, codes)
            compared += int(packed.size + back.size)
    J.report("pack+unpack", case=f"device-pointers-skew{skew}", compared=compared, mismatches=0)


@pytest.mark.parametrize("bits", [1, 5, 8, 10, 13, 17, 24])
def test_device_packer_writes_only_the_low_bits_of_a_code(bits):
    """The device forms cannot raise as containers.pack_codes does (BitPacker.cs:70-76): the header promises that the low `bits` bits
    are written and nothing else.  -1, 1 << bits and 2^40 + 5 among valid neighbours: the neighbours' bits are unchanged."""
    K, T = 3, 5
    mask = (1 << bits) - 1
    stream = np.random.default_rng(bits).integers(0, 1 << bits, (3, K * T), dtype=np.int64)
    stream[0, 4], stream[1, 7], stream[2, 14], stream[2, 0] = -1, 1 << bits, 2 ** 40 + 5, -(2 ** 40)
    packed = _pack_dev(J.to_codes(stream, K, T), bits, skew=1)
    assert np.array_equal(packed, J.ref_pack_rows(stream & mask, bits))
    assert np.array_equal(_unpack_dev(packed, K, T, bits), J.to_codes(stream & mask, K, T))
    with pytest.raises(ValueError):
        containers.pack_codes(J.to_codes(stream, K, T), bits)
    J.report("pack", case=f"low-bits-only-bits{bits}", compared=int(packed.size), mismatches=0)


def test_pack_refusals_leave_the_outputs_untouched_and_the_device_usable():
    lib = _lib.lib()
    B, K, T, bits = 2, 3, 5, 10
    nbytes = lib.nc_packed_bytes(K * T, bits)
    dcodes, dpacked = J.Canvas(np.int64, B * K * T), J.Canvas(np.uint8, B * nbytes)
    hcodes, hpacked = np.full(B * K * T, J.I64_CANARY, np.int64), np.full(B * nbytes, J.U8_CANARY, np.uint8)
    forms = ((lib.nc_pack_codes_dev, dcodes.ptr, dpacked.ptr, (None,)), (lib.nc_unpack_codes_dev, dpacked.ptr, dcodes.ptr, (None,)),
             (lib.nc_pack_codes, hcodes.ctypes.data, hpacked.ctypes.data, ()), (lib.nc_unpack_codes, hpacked.ctypes.data, hcodes.ctypes.data, ()))
    calls = 0
    for fn, src, dst, tail in forms:
        good = dict(dev=0, src=src, B=B, K=K, T=T, bits=bits, dst=dst)
        for bad in (dict(bits=0), dict(bits=25), dict(bits=-3), dict(B=0), dict(K=0), dict(T=0), dict(B=-1), dict(K=-1), dict(T=-1),
                    dict(src=None), dict(dst=None), dict(dev=999), dict(dev=-1)):
            assert fn(*dict(good, **bad).values(), *tail) != OK, (fn.__name__, bad)
            assert lib.nc_last_error()
            calls += 1
    assert dcodes.untouched() and dpacked.untouched()
    assert (hcodes == J.I64_CANARY).all() and (hpacked == J.U8_CANARY).all()
    stream = np.random.default_rng(9).integers(0, 1 << bits, (B, K * T), dtype=np.int64)      # one valid call of each form follows
    codes = J.to_codes(stream, K, T)
    want = J.ref_pack_rows(stream, bits)
    assert np.array_equal(containers.pack_codes(codes, bits), want) and np.array_equal(containers.unpack_codes(want, K, T, bits), codes)
    assert np.array_equal(_pack_dev(codes, bits), want) and np.array_equal(_unpack_dev(want, K, T, bits), codes)
    J.report("refusals", case="nc_pack", compared=calls, mismatches=0)
