"""Which kernel runs which config, and the dataset images, without a GPU.

ce_create plans before it touches the device (csrc/engine_plan.h); the
library's test hooks ce_test_plan and ce_test_dataset_image run the plan and
the host-side image builders alone.

The selection table below is transcribed from the kernel-name assertions of
the GPU suite (test_gpu_paths, test_gpu_mfma, test_gpu_mlp, test_gpu_persist,
test_gpu_lr_tiers, test_gpu_parity, test_gpu_bench_sizes): the same config,
the same CE_* switches, the same expected string.  The CE_PAIR_U rows, which
no GPU test pins by name, follow the instance naming of DESIGN.md 3.2
(optimize_pair_kernel<T, F, U>, optimize_step_kernel<T, F, K, STAGED>).
The image layouts are restated in numpy from the layout comments of
optimize_kernels.h (row_stride, signed_rows), optimize_mfma_kernel.h
(gen_stride, gen_rows_padded) and mlp_kernels.h (MlpArgs::Xs).
"""
import ctypes

import numpy as np
import pytest

from custom_envs_amd import _native
from custom_envs_amd.engine import make_config

CE_SWITCHES = ('CE_GENERIC', 'CE_LR_MFMA', 'CE_PAIR_U', 'CE_MLP_NET', 'CE_MLP_SPLIT',
               'CE_MLP_PHASES', 'CE_NO_STAGE', 'CE_LR_WAVES', 'CE_GEN_TAIL', 'CE_GEN_CAT',
               'CE_LR_MODE', 'CE_MANY_DIRECT')


@pytest.fixture(autouse=True)
def _clean_switches(monkeypatch):
    for name in CE_SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _lib():
    lib = _native.load()
    lib.ce_test_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_char_p,
                                 ctypes.c_char_p, ctypes.c_int32]
    lib.ce_test_plan.restype = ctypes.c_int
    lib.ce_test_dataset_image.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_void_p, ctypes.c_int64]
    lib.ce_test_dataset_image.restype = ctypes.c_int64
    return lib


def _plan(cfg, labels=None, env=None, monkeypatch=None):
    """(status, step kernel, K-step kernel) of ce_test_plan under `env`."""
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if labels is None:
        labels = np.arange(cfg.n_rows, dtype=np.int32) % max(cfg.n_classes, 1)
    labels = np.ascontiguousarray(labels, np.int32)
    step, many = ctypes.create_string_buffer(128), ctypes.create_string_buffer(128)
    rc = _lib().ce_test_plan(ctypes.byref(cfg), labels.ctypes.data, step, many, 128)
    return rc, step.value.decode(), many.value.decode()


def _mfma_flags(generic=False, lr=False, lr_waves=0, gen_tail=1, lr_mode=3, cat=False):
    """The switches test_gpu_mfma._engine sets around every engine."""
    return {'CE_GENERIC': '1' if generic else '0', 'CE_LR_MFMA': '1' if lr else '0',
            'CE_LR_WAVES': str(lr_waves), 'CE_GEN_TAIL': str(gen_tail),
            'CE_LR_MODE': str(lr_mode), 'CE_GEN_CAT': '1' if cat else '0'}


def _lin(N, F, K, E, B=None, precision='f64'):
    return dict(n_rows=N, n_features=F, n_classes=K, num_envs=E, batch_size=B, precision=precision)


def _mlp(N, F, K, E, B, hidden=64):
    return dict(n_rows=N, n_features=F, n_classes=K, num_envs=E, batch_size=B, model='mlp',
                hidden=hidden)


# (config, switches, how to compare, expected step kernel, expected K-step kernel or None)
TABLE = []


def _case(cfg, env, how, step, many=None):
    TABLE.append((cfg, env, how, step, many))


# ---- test_gpu_paths.py: test_unstaged_register_kernel
for _shape, _rows in (((10, 2), 200), ((10, 3), 150)):
    for _b in (None, 32):
        for _prec, _dt in (('f64', 'double'), ('f32', 'float')):
            _case(_lin(_rows, _shape[0], _shape[1], 21, _b, _prec),
                  {'CE_PAIR_U': '2', 'CE_NO_STAGE': '1'}, 'eq',
                  'optimize_step_kernel<%s,%d,%d,false>' % (_dt, _shape[0], _shape[1]))
# ---- test_gpu_mfma.py
_case(_lin(240, 49, 10, 1), {}, 'eq', 'optimize_cat_kernel<13,true,10>')   # the IDX fixture via make()
for _b in (None, 32, 100):
    _case(_lin(1000, 49, 10, 13, _b), _mfma_flags(), 'eq', 'optimize_mfma_kernel<13>')
for _tail in (1, 0):
    for (_f, _k), _name in (((4, 3), 'optimize_mfma_kernel<1>'), ((17, 2), 'optimize_mfma_kernel<5>'),
                            ((33, 7), 'optimize_mfma_kernel<9>'), ((64, 16), 'optimize_mfma_kernel<16>'),
                            ((49, 10), 'optimize_mfma_kernel<13>'), ((1, 5), 'optimize_mfma_kernel<1>')):
        _case(_lin(300, _f, _k, 9), _mfma_flags(generic=True, gen_tail=_tail), 'eq', _name)
for _b in (None, 32):
    _case(_lin(256, 10, 2, 10, _b), _mfma_flags(generic=True), 'eq', 'optimize_mfma_kernel<3>')
for _waves in (8, 4, 16):
    for _n, _f, _e in ((256, 10, 37), (200, 1, 16), (203, 13, 17), (1000, 16, 5), (4000, 4, 3),
                       (256, 5, 1), (384, 7, 21), (512, 3, 33), (1024, 10, 18)):
        _case(_lin(_n, _f, 2, _e), _mfma_flags(lr=True, lr_waves=_waves), 'startswith',
              'optimize_lr_mfma_kernel<%d,' % ((_f + 3) // 4))
for _mode in (0, 1, 2):
    for _waves in (4, 8):
        _case(_lin(256, 10, 2, 35), _mfma_flags(lr=True, lr_waves=_waves, lr_mode=_mode), 'eq',
              'optimize_lr_mfma_kernel<3,%d,%d>' % (_mode, _waves))
_case(_lin(256, 10, 2, 64), _mfma_flags(lr=True), 'contains', 'lr_mfma')
_case(_lin(256, 10, 2, 64), _mfma_flags(lr=False), 'lacks', 'lr_mfma')
for _n in (256, 203):
    _case(_lin(_n, 10, 2, 19), _mfma_flags(lr=True), 'contains', 'lr_mfma')
    _case(_lin(_n, 10, 2, 19), _mfma_flags(lr=False), 'lacks', 'lr_mfma')
_case(_lin(60000, 49, 10, 9), _mfma_flags(cat=True), 'eq', 'optimize_cat_kernel<13,true,10>')
_case(_lin(60000, 49, 10, 9), _mfma_flags(cat=False), 'eq', 'optimize_mfma_kernel<13>')
for (_f, _k, _n), _name in (((49, 10, 1000), 'optimize_cat_kernel<13,true,10>'),
                            ((17, 10, 300), 'optimize_cat_kernel<5,true,10>'),
                            ((16, 10, 203), 'optimize_cat_kernel<4,false,10>'),
                            ((12, 3, 300), 'optimize_cat_kernel<3,false,3>'),
                            ((32, 16, 130), 'optimize_cat_kernel<8,false,16>')):
    _case(_lin(_n, _f, _k, 13), _mfma_flags(cat=True), 'eq', _name)
# ---- test_gpu_mlp.py
_case(_mlp(1024, 784, 10, 3, 32), {}, 'eq', 'mlp_step_kernel')
_case(_mlp(1024, 784, 10, 4096, 32), {}, 'eq', 'mlp_step_kernel')
_case(_mlp(256, 64, 10, 37, 32), {}, 'eq', 'mlp_step_kernel')
_case(_mlp(256, 64, 10, 37, 32), {'CE_MLP_SPLIT': '1'}, 'eq', 'mlp_train_kernel+mlp_info_kernel')
for _b in (16, 32, 100):
    _case(_mlp(1024, 784, 10, 3, _b, (256, 256)), {}, 'eq', 'net<784,256,256,10>:mfma')
_case(_mlp(128, 16, 10, 5, 20, (96, 32, 48)), {}, 'startswith', 'net<')
_case(_mlp(128, 16, 10, 5, None, (40,)), {}, 'startswith', 'net<')
_case(_mlp(128, 16, 10, 5, 32, (64,)), {'CE_MLP_NET': '1'}, 'startswith', 'net<')
_case(_mlp(128, 16, 10, 5, 24, (33, 7)), {}, 'startswith', 'net<')
for _k in (16, 17, 32):
    _case(_mlp(192, 40, _k, 3, 24, (64, 48)), {}, 'endswith', ':mfma')
_case(_mlp(128, 16, 10, 3, 24, (300,)), {}, 'eq', 'net<16,300,10>:wide')
_case(_mlp(128, 16, 10, 3, None, (260, 300)), {}, 'eq', 'net<16,260,300,10>:wide')
_case(_mlp(128, 16, 10, 3, 32, (512, 40, 33)), {}, 'eq', 'net<16,512,40,33,10>:wide')
_case(_mlp(128, 16, 10, 70, 24, (300,)), {}, 'eq', 'net<16,300,10>:wide')
_case(_mlp(1024, 784, 10, 2, 32, (512,)), {}, 'eq', 'net<784,512,10>:wide')
_case(_mlp(128, 16, 10, 3, 20, (96, 32, 48)), {}, 'endswith', ':mfma')
_case(_mlp(128, 16, 10, 3, None, (256, 256)), {}, 'endswith', ':mfma')
# ---- test_gpu_persist.py (set_persistent(False) reports the step kernel)
_case(_lin(256, 10, 2, 4096), {}, 'eq', 'optimize_lr_mfma_kernel<3,3,4>',
      'optimize_lr_persist_ws_kernel<3,4,false>')
for _n, _f, _name in ((64, 10, 'optimize_lr_persist_ws_kernel<3,1,false>'),
                      (40, 10, 'optimize_lr_persist_ws_kernel<3,1,true>'),
                      (100, 4, 'optimize_lr_persist_ws_kernel<1,2,true>'),
                      (128, 16, 'optimize_lr_persist_ws_kernel<4,2,false>'),
                      (192, 6, 'optimize_lr_persist_ws_kernel<2,4,true>'),
                      (256, 8, 'optimize_lr_persist_ws_kernel<2,4,false>'),
                      (512, 7, 'optimize_lr_persist_kernel<2,8,false,4>'),
                      (300, 13, 'optimize_lr_persist_kernel<4,8,true,4>')):
    _case(_lin(_n, _f, 2, 37), {}, 'startswith', 'optimize_lr_mfma_kernel<', _name)
for _n, _f in ((100, 4), (192, 6), (256, 8), (40, 10), (128, 16)):
    _case(_lin(_n, _f, 2, 37), {'CE_LR_WAVES': '4'}, 'endswith', ',4>')
# ---- test_gpu_lr_tiers.py
for _n, _e in ((64, 16), (64, 17), (256, 16), (256, 17), (256, 32), (250, 16)):
    _case(_lin(_n, 10, 2, _e), {'CE_LR_WAVES': '4'}, 'endswith', ',4>')
# ---- test_gpu_parity.py
for _e in (4096, 512, 32768):
    _case(_lin(256, 10, 2, _e), {}, 'eq', 'optimize_lr_mfma_kernel<3,3,4>')
# ---- test_gpu_bench_sizes.py
_case(_lin(256, 10, 2, 1024, None, 'f32'), {}, 'startswith', 'optimize_pair_kernel<float,10,')
_case(_lin(60000, 49, 10, 4096), {}, 'eq', 'optimize_cat_kernel<13,true,10>')
_case(_mlp(1024, 784, 10, 1024, 32, (256, 256)), {}, 'eq', 'net<784,256,256,10>:mfma')
# ---- the switches no GPU test pins by name (DESIGN.md 3.2's instance names)
_case(_lin(256, 10, 2, 8), {'CE_LR_MFMA': '0'}, 'eq', 'optimize_pair_kernel<double,10,2>')
_case(_lin(256, 10, 2, 8), {'CE_PAIR_U': '2'}, 'eq', 'optimize_pair_kernel<double,10,2>')
_case(_lin(256, 10, 2, 8), {'CE_PAIR_U': '1'}, 'eq', 'optimize_pair_kernel<double,10,1>')
_case(_lin(256, 10, 2, 8), {'CE_PAIR_U': '0'}, 'eq', 'optimize_step_kernel<double,10,2,true>')
_case(_lin(256, 10, 2, 8, 32), {}, 'eq', 'optimize_pair_kernel<double,10,2>')
_case(_lin(256, 10, 2, 8, None, 'f32'), {}, 'eq', 'optimize_pair_kernel<float,10,1>')
_case(_lin(256, 16, 2, 8, 32), {}, 'eq', 'optimize_step_kernel<double,16,2,true>')
_case(_lin(8, 3, 3, 4, 4), {}, 'eq', 'optimize_step_kernel<double,3,3,true>')
_case(_lin(8, 3, 3, 4, 4), {'CE_GENERIC': '1'}, 'eq', 'optimize_mfma_kernel<1>')
_case(_lin(8, 3, 3, 4), {'CE_GENERIC': '1'}, 'eq', 'optimize_mfma_kernel<1>')
_case(_lin(300, 12, 3, 13), {}, 'eq', 'optimize_cat_kernel<3,false,3>')
_case(_lin(300, 12, 3, 13), {'CE_GEN_CAT': '0'}, 'eq', 'optimize_mfma_kernel<3>')
_case(_lin(256, 10, 2, 8), {'CE_GENERIC': '1'}, 'eq', 'optimize_mfma_kernel<3>')
_case(_mlp(128, 16, 10, 4, 32), {'CE_MLP_PHASES': 'train'}, 'eq', 'mlp_train_kernel+mlp_info_kernel')
_case(_lin(256, 10, 2, 8), {'CE_LR_MODE': '1', 'CE_LR_WAVES': '8'}, 'eq',
      'optimize_lr_mfma_kernel<3,1,8>')


def _id(case):
    cfg, env, _, step, _ = case
    shape = '%dx%dx%d' % (cfg['n_rows'], cfg['n_features'], cfg['n_classes'])
    extra = [str(cfg[k]) for k in ('batch_size', 'precision', 'hidden') if cfg.get(k) not in (None, 'f64')]
    flags = ['%s=%s' % (k[3:], v) for k, v in sorted(env.items())]
    return '-'.join([shape, 'E%d' % cfg['num_envs']] + extra + flags)


@pytest.mark.parametrize('case', TABLE, ids=_id)
def test_selection_table(case, monkeypatch):
    kwargs, env, how, step, many = case
    rc, got_step, got_many = _plan(make_config(**kwargs), env=env, monkeypatch=monkeypatch)
    assert rc == _native.CE_OK
    if how == 'eq':
        assert got_step == step
    elif how == 'startswith':
        assert got_step.startswith(step)
    elif how == 'endswith':
        assert got_step.endswith(step)
    elif how == 'contains':
        assert step in got_step
    else:
        assert step not in got_step
    if many is not None:
        assert got_many == many
    elif not got_step.startswith('optimize_lr_mfma_kernel'):
        assert got_many == got_step      # no K-step kernel off the two-class MFMA path


def test_every_path_is_covered():
    families = {'optimize_step_kernel': 0, 'optimize_pair_kernel': 0, 'optimize_mfma_kernel': 0,
                'optimize_cat_kernel': 0, 'optimize_lr_mfma_kernel': 0, 'mlp_step_kernel': 0,
                'net<': 0}
    for _, _, how, step, _ in TABLE:
        for name in families:
            if how != 'lacks' and step.startswith(name):
                families[name] += 1
    assert all(families.values()), families


def test_persistent_kernel_needs_few_rows():
    """N <= 512 rows (test_gpu_persist.py's forms); past it the K-step call
    runs the step kernel."""
    rc, step, many = _plan(make_config(**_lin(1024, 10, 2, 18)))
    assert rc == _native.CE_OK and many == step and step.startswith('optimize_lr_mfma_kernel<3,')


# ---- refusals: the hook gives ce_create's code (test_native_abi.py, abi_driver.cpp)
_BASE = dict(n_rows=128, n_features=16, n_classes=10, num_envs=2, batch_size=32)
_MLP_BASE = dict(n_rows=128, n_features=16, n_classes=10, num_envs=1, batch_size=32, model='mlp')


def _refusals():
    def cfg(base, **change):
        c = make_config(**base)
        for k, v in change.items():
            if k == 'hidden':
                for i, w in enumerate(v):
                    c.hidden[i] = w
            else:
                setattr(c, k, v)
        return c
    yield 'abi', cfg(_BASE, abi_version=999), None, _native.CE_EINVAL
    yield 'batch', cfg(_BASE, batch_size=129), None, _native.CE_EINVAL
    yield 'max_steps', cfg(_BASE, max_steps=0), None, _native.CE_EINVAL
    labels = np.ones(128, np.int32)
    labels[5] = 10
    yield 'label', cfg(_BASE), labels, _native.CE_EINVAL
    yield 'f65', cfg(_BASE, n_features=65), None, _native.CE_EUNSUPPORTED
    yield 'f65k5', make_config(4, 65, 5, 1, 4), None, _native.CE_EUNSUPPORTED
    yield 'mlp-k33', cfg(_MLP_BASE, n_classes=33), None, _native.CE_EUNSUPPORTED
    yield 'mlp-5-layers', cfg(_MLP_BASE, n_layers=5), None, _native.CE_EUNSUPPORTED
    yield 'mlp-f64', cfg(_MLP_BASE, precision=_native.CE_F64), None, _native.CE_EUNSUPPORTED
    yield 'mlp-9000', cfg(_MLP_BASE, n_layers=2, hidden=(9000, 64)), None, _native.CE_EUNSUPPORTED
    yield 'mlp-width-0', cfg(_MLP_BASE, n_layers=2, hidden=(0, 64)), None, _native.CE_EINVAL


@pytest.mark.parametrize('name,cfg,labels,code', [pytest.param(*r, id=r[0]) for r in _refusals()])
def test_refusals_match_ce_create(name, cfg, labels, code):
    lib = _lib()
    if labels is None:
        labels = np.arange(cfg.n_rows, dtype=np.int32) % cfg.n_classes
    features = np.zeros((max(cfg.n_rows, 1), max(cfg.n_features, 1)))
    handle = ctypes.c_void_p()
    rc_create = lib.ce_create(ctypes.byref(cfg), features.ctypes.data, labels.ctypes.data,
                              ctypes.byref(handle))
    text_create = lib.ce_last_error()
    rc_plan, _, _ = _plan(cfg, labels)
    assert rc_create == code and rc_plan == code
    assert lib.ce_last_error() == text_create and text_create
    assert lib.ce_test_dataset_image(ctypes.byref(cfg), features.ctypes.data, labels.ctypes.data,
                                     None, 0) == code


def test_null_arguments():
    lib = _lib()
    assert lib.ce_test_plan(None, None, None, None, 0) == _native.CE_EINVAL
    assert lib.ce_test_dataset_image(None, None, None, None, 0) == _native.CE_EINVAL


# ---- the dataset images against numpy restatements of their layouts
def _image(cfg, features, labels, env=None, monkeypatch=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    lib = _lib()
    features = np.ascontiguousarray(features, np.float64)
    labels = np.ascontiguousarray(labels, np.int32)
    size = lib.ce_test_dataset_image(ctypes.byref(cfg), features.ctypes.data, labels.ctypes.data,
                                     None, 0)
    assert size > 0
    out = np.full(size + 16, 0xAB, np.uint8)            # a guard past the image
    assert lib.ce_test_dataset_image(ctypes.byref(cfg), features.ctypes.data, labels.ctypes.data,
                                     out.ctypes.data, size) == size
    assert np.all(out[size:] == 0xAB)
    short = np.full(size, 0xAB, np.uint8)               # no room: the size, nothing written
    assert lib.ce_test_dataset_image(ctypes.byref(cfg), features.ctypes.data, labels.ctypes.data,
                                     short.ctypes.data, size - 1) == size
    assert np.all(short == 0xAB)
    return out[:size]


def _data(N, F, K, seed, labels=None):
    rs = np.random.RandomState(seed)
    x = rs.normal(0, 1, (N, F))
    y = rs.randint(0, K, N) if labels is None else np.asarray(labels)
    return x, y.astype(np.int32)


def _align16(n):
    return (n + 15) // 16 * 16


def _register_blob(x, y, K, dtype):
    """[rows | labels]: rows padded with zeros to an odd number of 16-byte
    units, two-class rows times s_y = +1 (y = 0) / -1 (y = 1), then the int32
    labels at the next 16-byte boundary, the whole padded to 16 bytes."""
    N, F = x.shape
    tsize = np.dtype(dtype).itemsize
    units = (F * tsize + 15) // 16
    RS = (units if units % 2 else units + 1) * 16 // tsize
    rows = np.zeros((N, RS), dtype)
    fold = K == 2 and F + 2 <= 32
    rows[:, :F] = np.where((y != 0)[:, None] & fold, -x, x).astype(dtype)
    xbytes = _align16(rows.nbytes)
    blob = np.zeros(_align16(xbytes + 4 * N), np.uint8)
    blob[:rows.nbytes] = rows.view(np.uint8).ravel()
    blob[xbytes:xbytes + 4 * N] = y.astype(np.int32).view(np.uint8)
    return blob


@pytest.mark.parametrize('precision,dtype', [('f64', np.float64), ('f32', np.float32)])
def test_register_image_pads(precision, dtype):
    """F = 3, K = 3, N = 5: the row stride pad (6 doubles / 4 floats per
    3-feature row) and the pad after the 20 label bytes."""
    x, y = _data(5, 3, 3, 1)
    got = _image(make_config(5, 3, 3, 4, precision=precision), x, y)
    want = _register_blob(x, y, 3, dtype)
    assert got.size == want.size == (5 * 6 * 8 + 32 if precision == 'f64' else 5 * 4 * 4 + 32)
    assert np.array_equal(got, want)


def test_register_image_sign_fold(monkeypatch):
    """F = 2, K = 2, mixed labels (the register path: CE_LR_MFMA=0)."""
    x, y = _data(5, 2, 2, 2, labels=[0, 1, 1, 0, 1])
    got = _image(make_config(5, 2, 2, 4), x, y, {'CE_LR_MFMA': '0'}, monkeypatch)
    assert np.array_equal(got, _register_blob(x, y, 2, np.float64))
    rows = got[:5 * 2 * 8].view(np.float64).reshape(5, 2)     # one 16-byte unit per row
    assert np.array_equal(rows[1], -x[1]) and np.array_equal(rows[0], x[0])


def _gen_image(x, y):
    """[Npad][16 FT + 2] float64: the features, zeros, the label as a double
    in the last column; rows N.. pad to a multiple of 64 rows with label -1."""
    N, F = x.shape
    RS = 16 * ((F + 15) // 16) + 2
    img = np.zeros(((N + 63) // 64 * 64, RS))
    img[:N, :F] = x
    img[:N, RS - 1] = y
    img[N:, RS - 1] = -1.0
    return img


@pytest.mark.parametrize('n_rows', [1, 65])
def test_gen_image(n_rows):
    """F = 17 (two feature tiles), K = 5; one row, and one row past a whole
    64-row block (pad rows carry label -1)."""
    x, y = _data(n_rows, 17, 5, 3)
    got = _image(make_config(n_rows, 17, 5, 4), x, y).view(np.float64)
    want = _gen_image(x, y)
    assert want.shape == ((1 if n_rows == 1 else 2) * 64, 34)
    assert np.array_equal(got.reshape(want.shape), want)


def _mlp_image(x):
    """The float32 rows, then Xs: [N/32 tiles][F/8 chunks][64 lanes][4],
    element j of lane l = X[32 t + (l & 31)][8 c + 4 (l >> 5) + j]."""
    x32 = x.astype(np.float32)
    N, F = x32.shape
    t, c, l, j = np.ix_(np.arange(N // 32), np.arange(F // 8), np.arange(64), np.arange(4))
    xs = x32[32 * t + (l & 31), 8 * c + 4 * (l >> 5) + j]
    return np.concatenate([x32.ravel(), xs.ravel()])


@pytest.mark.parametrize('n_features,n_rows', [(8, 64), (16, 128)])
def test_fused_mlp_image(n_features, n_rows):
    """The smallest shapes the fused kernel takes (F % 8 == 0, N % 64 == 0)."""
    x, y = _data(n_rows, n_features, 10, 4)
    cfg = make_config(**_mlp(n_rows, n_features, 10, 4, 32))
    assert _plan(cfg)[1] == 'mlp_step_kernel'
    got = _image(cfg, x, y).view(np.float32)
    assert np.array_equal(got, _mlp_image(x))


def test_net_image_is_the_float32_rows(monkeypatch):
    x, y = _data(128, 16, 10, 5)
    got = _image(make_config(**_mlp(128, 16, 10, 4, 32)), x, y, {'CE_MLP_NET': '1'}, monkeypatch)
    assert np.array_equal(got.view(np.float32), x.astype(np.float32).ravel())
