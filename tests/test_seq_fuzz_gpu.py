"""Call sequences across entry points, streams and objects (tests/seq_fuzz.py): each program is
enqueued as written, synchronised once at its end and then compared step by step with the oracles
the per-feature tests use (run_program's docstring: kernel names, every output word, every guard
band and input, the recomputed count).  The same seeds run again with the exact kernel as the
starting state, and two of them with every caller pointer word-aligned only (dev_arena skew; the
u_a of tfhe_amd_keyswitch_batch_dev keeps the 16 bytes include/tfhe_amd.h asks for).

The oracle's results of a seed are computed once per session and shared by the forms of that seed."""
import pytest

import seq_fuzz as SF

pytestmark = pytest.mark.gpu


def _run(ctx, keyset, okey, seed, start_kernel, skew=False):
    t = SF.run_program(SF.make_program(seed, start_kernel), ctx, keyset, okey, skew=skew)
    print(f"seq fuzz seed {seed}, start kernel {start_kernel}, skew {skew}: oracle {t['oracle_s']:.2f} s, "
          f"solo runs {t['solo_s']:.2f} s, program {t['program_s']:.3f} s")


@pytest.mark.parametrize("seed", SF.SEEDS)
def test_program(ctx, keyset, okey, seed):
    _run(ctx, keyset, okey, seed, 0)


@pytest.mark.parametrize("seed", SF.SEEDS)
def test_program_from_the_exact_kernel(ctx, keyset, okey, seed):
    """select_kernel(4) is the starting state and the program's kernel steps flip to 0 and back"""
    _run(ctx, keyset, okey, seed, 4)


@pytest.mark.parametrize("seed", SF.SKEW_SEEDS)
def test_program_on_word_aligned_pointers(ctx, keyset, okey, seed):
    _run(ctx, keyset, okey, seed, 0, skew=True)
