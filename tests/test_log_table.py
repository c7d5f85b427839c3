"""The two-class kernels' table logarithm (log_pos_tab) and batched softmax
reciprocal (lr_post4) restated in C on the host
(tests/log_table/tlog.c: gcc, -ffp-contract=off, explicit fma()).

log_pos_tab over the committed table against logl: 2e6 log-uniform x in
[1e-256, 1], 2e5 values 1 - 10^-k, the values 1, 1 + 16e-16, 0.5 and 1e-256,
and every table boundary 2^(-j/2048) (with both neighbours) at the index as
found and forced one off either way.  Bounds: 2 ulp where |log x| >= 0.5,
2.5e-16 absolute below.  Measured: 1.46 ulp and 1.10e-16; the forced-index
cases 1.34 ulp and 1.27e-16.

The batched reciprocal beside rcp_newton1, the hardware seed modelled as
exact 1/d times 1 +- 2^-24 and random between, d log-uniform in [1, 2^231]
in groups of four.  Bound: the batched form's worst error is at most
rcp_newton1's worst over the same inputs plus 2 ulp, every result finite at
the top of the range.  Measured: rcp_newton1 32.50 ulp, the batched form as
shipped (the third-order correction of the shared seed) 3.39 ulp; with one
Newton step on the product (CE_LR_RCPB_NEWTON=1) it would be 34.92, outside
the bound: each value carries four more roundings of up to one ulp of the
result, not three of half an ulp.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'custom_envs_amd', 'csrc')

pytestmark = pytest.mark.skipif(shutil.which('gcc') is None, reason='needs gcc')


@pytest.fixture(scope='module')
def tlog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('tlog') / 'tlog')
    subprocess.run(['gcc', '-O2', '-ffp-contract=off', '-I', CSRC,
                    os.path.join(ROOT, 'tests', 'log_table', 'tlog.c'), '-o', exe, '-lm'], check=True)
    return exe


def _run(exe, mode):
    out = subprocess.run([exe, mode], check=True, capture_output=True, text=True).stdout
    print(mode, out.strip())
    return out.split()


def test_table_log_accuracy(tlog):
    ulp, absolute, forced_ulp, forced_abs = map(float, _run(tlog, 'log'))
    assert ulp <= 2.0, ulp
    assert absolute <= 2.5e-16, absolute
    assert forced_ulp <= 2.0, forced_ulp
    assert forced_abs <= 2.5e-16, forced_abs


def test_batched_reciprocal_accuracy(tlog):
    single, batched, finite, one_step = _run(tlog, 'rcp')
    print('rcp_newton1 %s ulp, batched %s ulp, batched with one Newton step %s ulp'
          % (single, batched, one_step))
    assert finite == '1'
    assert float(batched) <= float(single) + 2.0, (single, batched)


def test_kernels_share_one_post():
    """The three two-class kernels batch the same four values: one lr_post4
    in optimize_lr_mfma.h, none of their own."""
    mfma = open(os.path.join(CSRC, 'optimize_lr_mfma.h')).read()
    persist = open(os.path.join(CSRC, 'optimize_lr_persist.h')).read()
    assert mfma.count('void lr_post4(') == 1
    assert 'rcp_newton1(1.0 +' not in persist and 'auto post =' not in persist
    assert persist.count('lr_post4(') == 2 and persist.count('lr_log(') == 4
