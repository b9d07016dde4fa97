"""CPU: what bench.py prints and writes, without running a step.  The printed result line is read back from a bounded tail
of the output, so it must stay short and parse; --dump-outputs must write the step's arrays in float64, sampled the same
way on every run when they exceed the size limit; a plain run measures the headline figure alone, --full everything else."""
import json
import os

import numpy as np
import torch

import bench

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_result_line_is_short_and_keeps_the_contract_keys():
    # a full result object of the default invocation, as recorded in profiles/ (every operating point, per-kernel maps)
    with open(os.path.join(REPO, 'profiles', 'r06_bench.json')) as f:
        full = json.loads(f.read().strip().splitlines()[-1])
    assert len(json.dumps(full)) > 16000
    line = json.dumps(bench.compact_line(bench.order_line(full)))
    assert len(line) < 4096, len(line)
    back = json.loads(line)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'roofline', 'cpu_baseline'):
        assert back[k] == full[k], k
    assert list(back)[-1] == 'summary' and set(back['summary']) >= {'c3', 'c5', 'b8', 'fp32', 'fp16'}


def test_dump_outputs_writes_float64_and_a_fixed_sample(tmp_path):
    g = torch.Generator().manual_seed(0)
    terms = {'full_loss': torch.tensor(1.5, dtype=torch.bfloat16), 'big': torch.randn(300, 300, generator=g), 'note': 'x'}
    for sub in ('a', 'b'):
        bench.dump_outputs(terms, str(tmp_path / sub), limit_bytes=2 * 64 * 1024)
    assert sorted(os.listdir(str(tmp_path / 'a'))) == ['big.npy', 'full_loss.npy']
    loss = np.load(str(tmp_path / 'a' / 'full_loss.npy'))
    assert loss.dtype == np.float64 and loss.shape == () and float(loss) == 1.5
    a, b = np.load(str(tmp_path / 'a' / 'big.npy')), np.load(str(tmp_path / 'b' / 'big.npy'))
    assert a.dtype == np.float64 and a.nbytes <= 64 * 1024 and a.size == 8192
    np.testing.assert_array_equal(a, b)
    assert np.isin(a, terms['big'].double().numpy().reshape(-1)).all()


EXTRAS = ('no_roofline', 'no_c3', 'no_c5', 'no_points', 'no_cpu_baseline')


def test_plain_run_measures_the_headline_figure_only():
    args = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not args.full and all(getattr(args, n) for n in EXTRAS)
    assert (args.steps, args.warmup, args.batch, args.seq, args.size, args.dtype) == (20, 5, 32, 30, 128, 'bf16')
    # what such a run prints: the contract keys, no roofline / baseline / summary of other operating points
    with open(os.path.join(REPO, 'profiles', 'r06_bench.json')) as f:
        full = json.loads(f.read().strip().splitlines()[-1])
    plain = {k: v for k, v in full.items() if k not in ('roofline', 'roofline_other_bound', 'cpu_baseline', 'c3', 'c3_clstm', 'c5',
                                                         'b8', 'fp32', 'fp16', 'summary', 'kernels_ms_per_step',
                                                         'kernel_groups_ms_per_step', 'kernel_groups_tflops')}
    back = json.loads(json.dumps(bench.compact_line(bench.order_line(plain))))
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert back[k] == full[k], k
    assert list(back)[:7] == ['metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step'] and 'summary' not in back


def test_full_run_keeps_every_extra_measurement_and_its_switches():
    args = bench.parse_args(['--full'])
    assert args.full and not any(getattr(args, n) for n in EXTRAS)
    args = bench.parse_args(['--full', '--no-c3', '--no-cpu-baseline'])
    assert args.no_c3 and args.no_cpu_baseline and not (args.no_roofline or args.no_c5 or args.no_points)
