"""CPU: ABI 9 -- the dropout key read from device memory (RFN_PATH_OPT_SEED_DEV, rfn_dropout_mask_dev).  Host-side checks only:
every call here is refused by its argument validation before anything is launched, so the fake device addresses are never
dereferenced."""
import ctypes as C

FAKE = 0x10000          # a non-null, 16-byte aligned "device address" for calls that must fail before using it


def native():
    import recurrent_fusion_network_amd._native as N
    return N


def test_abi_version_is_9():
    N = native()
    assert N.lib.rfn_abi_version() == 9 and N.ABI_VERSION == 9


def test_seed_dev_flag_is_one_free_bit_and_dims_keep_their_size():
    N = native()
    flag = N.PATH_OPT_SEED_DEV
    assert flag > 0 and flag & (flag - 1) == 0
    others = {k: getattr(N, k) for k in dir(N) if k.startswith('PATH_OPT_') and k != 'PATH_OPT_SEED_DEV'}
    assert len(others) >= 9
    for k, v in others.items():
        assert flag & v == 0, k
    assert flag == 256                       # the lowest bit the other options leave free
    assert C.sizeof(N.Dims) == 168 and N.Dims.path_flags.offset == 152 and N.Dims.probe_events.offset == 160


def test_dropout_mask_dev_is_exported_and_validates_like_dropout_mask():
    N = native()
    fn = N.lib.rfn_dropout_mask_dev
    assert 'rfn_dropout_mask_dev' in N.EXPORTS
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_uint64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
    ERR_SHAPE, ERR_ARG = -1, -5
    assert fn(None, 0, 16, 0.5, FAKE, None) == ERR_ARG          # NULL seed pointer
    assert fn(FAKE, 0, 16, 0.5, None, None) == ERR_ARG          # NULL output
    for n in (0, -3):
        assert fn(FAKE, 0, n, 0.5, FAKE, None) == ERR_SHAPE
        assert N.lib.rfn_dropout_mask(1, 0, n, 0.5, FAKE, None) == ERR_SHAPE
    assert fn(FAKE, 0, 16, 1.0, FAKE, None) == ERR_SHAPE == N.lib.rfn_dropout_mask(1, 0, 16, 1.0, FAKE, None)
    assert N.lib.rfn_dropout_mask(1, 0, 16, 0.5, None, None) == ERR_ARG


def test_path_entry_points_refuse_a_null_seed_address():
    N = native()
    kw = dict(M=2, R=16, A=16, E=16, T1=3, T2=3, K=20, V1=51, L=[5, 7], D=[24, 40], Fc=[24, 32], drop_lm=0.3)
    d = N.make_dims(path_flags=N.PATH_OPT_SEED_DEV, **kw)
    B, S = 2, 3
    ws = N.lib.rfn_decoder_ws_bytes(C.byref(d), B, S, 1)
    assert ws > 0
    # rfn_decoder_fwd(d, B, S, prm, comb, h0, c0, ids, ld_ids, log_prob, ws, ws_bytes, train, seed, stream)
    args = (C.byref(d), B, S, FAKE, FAKE, FAKE, FAKE, FAKE, S + 1, FAKE, FAKE, ws, 1)
    assert N.lib.rfn_decoder_fwd(*args, 0, None) == -5                      # flag set, seed address 0: RFN_ERR_ARG
    assert N.lib.rfn_decoder_fwd(*args, FAKE + 4, None) == -5               # not 8-byte aligned
    # ... and the other entry points that take (dims, seed) validate it the same way, before any launch
    assert N.lib.rfn_prefix_fwd(C.byref(d), B, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 40, 1, 0, None) == -5
    assert N.lib.rfn_decoder_bwd(C.byref(d), B, S, FAKE, FAKE, FAKE, FAKE, FAKE, S + 1, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE,
                                 ws, 0, None) == -5
    assert N.lib.rfn_decoder_step(C.byref(d), B, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None, 0, FAKE, 1 << 40, 0, 0, None) == -5
    # without the flag a zero seed is an ordinary key: the same call gets past the seed check (and is refused for its
    # workspace, still before any launch)
    d0 = N.make_dims(**kw)
    assert N.lib.rfn_decoder_fwd(C.byref(d0), B, S, FAKE, FAKE, FAKE, FAKE, FAKE, S + 1, FAKE, FAKE, 16, 1, 0, None) == -4
