"""The entry point's host-side pieces that need no GPU: the graph-or-eager runner of `train()` with a stand-in for the graphed iteration,
and the checkpoint pair on tiny modules."""
import logging
import os

import pytest
import torch

from golden_util import CFG_DIR


class _Graphed:
    """what the runner uses of a GraphedIteration: static_in, it_state, __call__, close; raises ``exc`` on call number ``fail_at``"""

    def __init__(self, inputs, fail_at=0, exc=None):
        self.static_in, self.it_state = [t.clone() for t in inputs], {}
        self.fail_at, self.exc, self.calls, self.closed = fail_at, exc, 0, 0

    def __call__(self, *inputs):
        self.calls += 1
        if self.calls == self.fail_at:
            raise self.exc
        self.it_state['i'] = self.calls % 2              # (the N_CRITIC counter moves as batches are stepped)
        return {'batch': inputs[0], 'by': 'graph'}

    def close(self):
        self.closed += 1


def _runner(fail_at=0, exc=None):
    import xmc_gan.train_gan as tg
    made, stepped = [], []

    def factory(step_fn, inputs):
        made.append(_Graphed(inputs, fail_at, exc))
        return made[-1]

    def step_fn(x, y, state):
        stepped.append((int(x[0]), dict(state)))
        return {'batch': x, 'by': 'eager'}

    return tg.IterationRunner(step_fn, logging.getLogger('runner-test'), use_graph=True, factory=factory), made, stepped


def _batch(i, n=2):
    return torch.full((n,), float(i)), torch.zeros(n, 3)


def test_runner_falls_back_to_eager_launches_on_a_failed_capture_only(caplog):
    from xmc_gan_amd.graph import CaptureFailed
    assert issubclass(CaptureFailed, RuntimeError)
    runner, made, stepped = _runner(3, CaptureFailed('OutOfMemoryError: no room'))
    with caplog.at_level(logging.INFO, logger='runner-test'):
        outs = [runner(_batch(i)) for i in range(5)]
    assert [o['by'] for o in outs] == ['graph', 'graph', 'eager', 'eager', 'eager']
    assert len(made) == 1 and made[0].calls == 3 and made[0].closed == 1           # not made again after the fallback
    assert [i for i, _ in stepped] == [2, 3, 4]                                    # the third batch is stepped exactly once
    assert stepped[0][1] == {'i': 0}                                               # ... from the state the graphed iterations left
    lines = [r.getMessage() for r in caplog.records]
    assert lines == ['hipGraph capture failed (OutOfMemoryError: no room); continuing with eager launches']
    assert not runner.hipgraph
    runner.close()
    assert made[0].closed == 1


def test_runner_lets_every_other_exception_through():
    runner, made, stepped = _runner(3, RuntimeError('a replay failed'))
    runner(_batch(0)), runner(_batch(1))
    with pytest.raises(RuntimeError, match='a replay failed') as e:
        runner(_batch(2))
    from xmc_gan_amd.graph import CaptureFailed
    assert not isinstance(e.value, CaptureFailed)
    assert stepped == [] and runner.hipgraph and made[0].closed == 0                # that batch is not run again with eager launches


def test_runner_sends_a_batch_of_another_shape_to_the_eager_path():
    runner, made, stepped = _runner()
    runner(_batch(0))
    out = runner(_batch(1, n=1))                     # (the last batch of a loader without drop_last)
    assert out['by'] == 'eager' and made[0].calls == 1 and [i for i, _ in stepped] == [1]
    assert stepped[0][1] == {'i': 1}                 # one counter for both paths
    assert runner(_batch(2))['by'] == 'graph' and made[0].calls == 2 and runner.hipgraph


def test_graphed_iteration_names_a_failed_capture(monkeypatch):
    """`GraphedIteration.__call__` wraps its capture, and nothing else, into CaptureFailed"""
    from xmc_gan_amd.graph import CaptureFailed, GraphedIteration

    def step_fn(x, state):
        raise ValueError('from a warm-up iteration')

    g = GraphedIteration(step_fn, (torch.zeros(2),), warmup=1)
    with pytest.raises(ValueError, match='from a warm-up iteration'):
        g(torch.zeros(2))

    def no_capture(phase):
        raise MemoryError('no room')

    monkeypatch.setattr(g, '_capture', no_capture)
    with pytest.raises(CaptureFailed, match='MemoryError: no room') as e:
        g(torch.zeros(2))
    assert isinstance(e.value.__cause__, MemoryError)


@pytest.mark.parametrize("max_steps", [None, 2])
def test_train_closes_the_runner_on_both_returns(monkeypatch, max_steps):
    import xmc_gan.train_gan as tg
    from xmc_gan.config import gan
    gan.reset_cfg()
    gan.cfg_from_file(os.path.join(CFG_DIR, "df_gan_damsm.yml"))
    gan.cfg.TRAIN.MAX_EPOCH = 1
    closed, made = [], []

    class Runner(tg.IterationRunner):
        def __init__(self, step_fn, logger, use_graph):
            super().__init__(step_fn, logger, True, factory=lambda fn, inputs: made.append(_Graphed(inputs)) or made[-1])

        def close(self):
            closed.append(self.hipgraph)
            super().close()

    monkeypatch.setattr(tg, 'IterationRunner', Runner)
    T = gan.cfg.TEXT.MAX_LENGTH
    loader = [(torch.zeros(2, 3, 8, 8), [(torch.ones(2, T, dtype=torch.int64), torch.tensor([3, 4]))], ['a', 'b']) for _ in range(3)]
    enc = tg.SyntheticTextEncoder(gan.cfg.TEXT.EMBEDDING_DIM, T, 1, torch.device('cpu'))
    netG, netD = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    last = tg.train(loader, None, 0, enc, netG, netD, None, None, logging.getLogger('train-test'), None, opts=tg.StepOptions(graph=True),
                    max_steps=max_steps)
    assert closed == [True] and made[0].closed == 1 and made[0].calls == (max_steps or 3)
    assert last['hipgraph'] is True and last['by'] == 'graph'


def _tiny():
    netG, netD = torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)
    optG, optD = torch.optim.Adam(netG.parameters(), lr=1e-2), torch.optim.Adam(netD.parameters(), lr=1e-2)
    return netG, netD, optG, optD


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_checkpoint_pair_round_trip_and_listing(tmp_path, mode):
    import xmc_gan.train_gan as tg
    from xmc_gan_amd import ops
    ops.set_precision(mode)
    try:
        torch.manual_seed(3)
        netG, netD, optG, optD = _tiny()
        for _ in range(2):
            optG.zero_grad(), optD.zero_grad()
            netD(netG(torch.randn(4, 3))).sum().backward()
            optG.step(), optD.step()
        tg.save_checkpoint(str(tmp_path), 7, netG, netD, optG, optD)
        assert sorted(os.listdir(tmp_path)) == ["netD_007.pth", "netG_007.pth", "optimizerD.pth", "optimizerG.pth"]       # no loss_scale.pth, no EMA
        fresh = _tiny()
        lines = []
        log = logging.getLogger('ckpt-test')
        monkey = logging.Handler()
        monkey.emit = lambda r: lines.append(r.getMessage())
        log.addHandler(monkey), log.setLevel(logging.INFO)
        try:
            tg.load_checkpoint(str(tmp_path), 7, *fresh, device=torch.device('cpu'), logger=log)
        finally:
            log.removeHandler(monkey)
        assert lines == ['Load models, epoch : 7']
        for new, old in zip(fresh[:2], (netG, netD)):
            assert all(torch.equal(a, b) for a, b in zip(new.state_dict().values(), old.state_dict().values()))
        for new, old in zip(fresh[2:], (optG, optD)):
            a, b = new.state_dict(), old.state_dict()
            assert a['param_groups'] == b['param_groups'] and a['state'].keys() == b['state'].keys() and len(a['state']) == 2
            for k in a['state']:
                assert all(torch.equal(torch.as_tensor(a['state'][k][n]), torch.as_tensor(b['state'][k][n])) for n in ('step', 'exp_avg', 'exp_avg_sq'))
    finally:
        ops.set_precision("bf16")
