"""Host-side checks of the narrow forward's plumbing: ksp.NarrowForm -- the five keywords narrow, narrow_rows, narrow32, narrow64, narrow_linear resolved once per
call -- against the expressions the host used inline before it, over the whole grid of keyword values; and KeyedLayer.forward against KeyedLayer.launch: the flag
word a planner is told is the flag word the forward runs, for every operator kind, contract and accepted keyword set.  No GPU, no built library."""
import itertools

import numpy as np
import pytest
import scipy.sparse
import torch

from keynet_amd import _capi
from keynet_amd import sparse as ksp
from keynet_amd import system as ksys
from keynet_amd.layer import KeyedLayer
from test_narrow_host import _tiny_conv

KEYWORDS = ('narrow', 'narrow_rows', 'narrow32', 'narrow64', 'narrow_linear')
GRID = [dict(zip(KEYWORDS, v)) for v in itertools.product((False, True, 'mfma'), (False, True), (False, True), (False, True, 'mfma'), (False, True))]


def _rule(n, kw, alone=False):
    """ksp._narrow_args on a keyword set: ('ok', (mode, rows)) or ('refused', message)."""
    try:
        return ('ok', ksp._narrow_args(n, kw['narrow'], kw['narrow_rows'], 'images', alone, narrow32=kw['narrow32'], narrow64=kw['narrow64'], narrow_linear=kw['narrow_linear']))
    except ValueError as e:
        return ('refused', str(e))


@pytest.mark.parametrize('n', [1, 8, 9, 32, 33, 64, 65])
def test_the_form_is_the_argument_rule_and_the_inline_expressions(n):
    for (kw, alone) in itertools.product(GRID, (False, True)):
        (verdict, value) = _rule(n, kw, alone)
        if verdict == 'refused':
            with pytest.raises(ValueError) as e:
                ksp.NarrowForm.of(n, alone=alone, **kw)
            assert str(e.value) == value, (n, kw, alone)
            continue
        form = ksp.NarrowForm.of(n, alone=alone, **kw)
        assert (form.mode, form.rows) == value and type(form.mode) is type(value[0]), (n, kw, alone)
        assert form.narrow32 is bool(kw['narrow32'] or kw['narrow64']) and form.narrow64 is bool(kw['narrow64']), (n, kw, alone)
        assert form.tile64 is (kw['narrow64'] == 'mfma' and n > 32) and form.linear is bool(kw['narrow_linear']), (n, kw, alone)
        # the keywords it hands back: the pinned surfaces' own, already normalised -- the same form again
        back = form.keywords()
        assert tuple(back) == KEYWORDS and back['narrow64'] == ksys.KeyedModel._narrow64_form(n, kw['narrow64']), (n, kw, alone)
        assert ksp.NarrowForm.of(n, alone=alone, **back) == form, (n, kw, alone)
    # without a batch (KeyedLayer.kernel / launch) nothing is refused: the same expressions, the tile asked for at whatever width the caller has in mind
    for kw in GRID:
        form = ksp.NarrowForm.of(None, **kw)
        assert form == (kw['narrow'] if kw['narrow'] == 'mfma' else bool(kw['narrow']), bool(kw['narrow_rows']), bool(kw['narrow32'] or kw['narrow64']), bool(kw['narrow64']),
                        kw['narrow'] == 'mfma' and kw['narrow64'] == 'mfma', bool(kw['narrow_linear'])), kw
    assert ksp.NarrowForm.of(None) == ksp.NarrowForm.of(5) == (False,) * 6


# -- KeyedLayer.forward and KeyedLayer.launch make the same thing of a keyword set -----------------------------------------------------------------------------
WIDTHS = (8, 32, 48)
MEASURED = dict(decided='mfma', gate_ratio=0.1, max_abs_x=2.0, measured_on_columns=4)
KEPT = dict(decided='exact', gate_ratio=0.9, max_abs_x=2.0, measured_on_columns=4)


def _operator(kind):
    W = _tiny_conv() if kind == 'conv' else ksp.SparseMatrix(scipy.sparse.random(12, 9, density=0.4, format='csr', dtype=np.float32, random_state=1))
    W._device_op = lambda device=None: 'handle'
    W._dense_device_op = lambda device=None: None
    return W


def _layer(kind, contract, record=None):
    """A keyed layer on the tiny operator: under the declared `contract`, or (record: 'none' | a narrow record) put on the matrix cores by a planted calibration."""
    c = KeyedLayer.fromoperator(_operator(kind), 'Conv2d' if kind == 'conv' else 'Linear', exact=False if record is not None else contract)
    if record is not None:
        c._contract_record = dict(decided='mfma', max_abs_x=1.0)
        if record != 'none':
            c._contract_record['narrow'] = dict(record)
        assert c.screened()
    return c


def _accepted(n, narrow_only=False):
    return [kw for kw in GRID if _rule(n, kw)[0] == 'ok' and (kw['narrow'] or not narrow_only)]


@pytest.fixture
def handed_down(monkeypatch):
    """What KeyedLayer.forward hands its operator: ksp._run_torchdot (the containers' torchdot look it up as a module global) records (W, exact, relu, keywords)."""
    calls = []

    def record(W, x, relu=False, exact=True, absmax=None, **kw):
        calls.append((W, exact, relu, kw))
        return torch.zeros((W.shape[0], x.shape[1]))
    monkeypatch.setattr(ksp, '_run_torchdot', record)
    return calls


def _forward_word(c, n, relu, kw, calls):
    """The flag word of the launch c.forward issues for n images under the keywords kw (None: not one launch)."""
    del calls[:]
    y = c.forward(torch.zeros((n, c.W.shape[1])), fuse_relu=relu, **kw)
    assert tuple(y.shape) == (n, c.W.shape[0]) and len(calls) == 1
    (W, exact, r, down) = calls[0]
    assert W is c.W and r == relu
    k = KeyedLayer.kernel(W, exact, r, None, **down)
    return None if k is None else k[1]


def _launch_word(c, relu, kw):
    la = c.launch(None, relu, **kw)
    return None if la is None else la.flags


CASES = ([('conv', contract, None) for contract in (True, False, 'bf16x3', 'split', 'auto')] + [('csr', contract, None) for contract in (True, False, 'bf16x3', 'split')] +
         [(kind, False, record) for kind in ('conv', 'csr') for record in (MEASURED, KEPT)])


@pytest.mark.parametrize('kind,contract,record', CASES, ids=lambda v: v if isinstance(v, str) else ('-' if v is None else v['decided'] if isinstance(v, dict) else str(v)))
def test_forward_and_launch_agree(kind, contract, record, handed_down):
    """Every accepted keyword set at 8, 32 and 48 images, with and without a fused ReLU.  The wide form (no keyword) of an 'auto' layer is left out: that forward calibrates,
    which is no matter of the narrow forms.  narrow64='mfma' asks launch() for the launch of 33 .. 64 columns, so below that width launch() is asked with what the forward
    of that width is: narrow64=True (KeyedModel._narrow64_form)."""
    seen = set()
    for n in WIDTHS:
        forms = _accepted(n, narrow_only=contract == 'auto')
        assert forms
        for (kw, relu) in itertools.product(forms, (False, True)):
            c = _layer(kind, contract, record)
            word = _forward_word(c, n, relu, kw, handed_down)
            assert word == _launch_word(c, relu, dict(kw, narrow64=ksys.KeyedModel._narrow64_form(n, kw['narrow64']))), (n, kw, relu, word)
            assert c._exact == (False if record is not None else c._exact_decl) and (record is None or c.narrow_record() == record)      # nothing decided, nothing recorded
            seen.add(word)
    if kind == 'conv':                                                   # the forms are told apart: the test is not comparing one word with itself
        want = _capi.KN_FLAG_NARROW_MFMA if (record == MEASURED or (record is None and contract in (False, 'bf16x3', 'split'))) else _capi.KN_FLAG_NARROW
        assert any(w is not None and w & want for w in seen) and any(w is not None and w & _capi.KN_FLAG_NARROW64 for w in seen)
        assert any(w is not None and w & _capi.KN_FLAG_NARROW64_MFMA for w in seen) == (contract in (False, 'bf16x3'))
    else:
        assert any(w & _capi.KN_FLAG_NARROW_ROWS for w in seen) and any(w & _capi.KN_FLAG_NARROW_LINEAR for w in seen)


def test_an_undecided_layer_without_a_narrow_form_differs_by_design(handed_down):
    """forward() runs it in the reference's order for this call; a planner is told it is not one launch yet.  Nothing is decided."""
    for n in WIDTHS:
        for (kw, relu) in itertools.product(_accepted(n, narrow_only=True), (False, True)):
            c = _layer('csr', 'auto')
            word = _forward_word(c, n, relu, kw, handed_down)
            assert handed_down[0][1] is True and word == _launch_word(_layer('csr', True), relu, kw), (n, kw, relu)
            assert c.launch(None, relu, **kw) is None and c._exact == 'auto'


def test_a_calibrated_layer_without_a_narrow_record_differs_by_design(handed_down, monkeypatch):
    """forward(narrow='mfma') measures the matrix-core narrow kernel on its batch and runs what the measurement says; a planner has no batch, measures nothing and is
    told the channel-lane kernel.  Beyond 32 images under narrow64='mfma' the wide decision covers the 64-column tile: nothing is measured, the two agree."""
    for (n, decided) in itertools.product(WIDTHS, ('mfma', 'exact')):
        for (kw, relu) in itertools.product([kw for kw in _accepted(n) if kw['narrow'] == 'mfma'], (False, True)):
            c = _layer('conv', False, 'none')
            measured = []
            monkeypatch.setattr(c, '_measure_narrow', lambda xt, r: measured.append((int(xt.shape[1]), r)) or dict(MEASURED, decided=decided))
            asked = dict(kw, narrow64=ksys.KeyedModel._narrow64_form(n, kw['narrow64']))
            before = _launch_word(c, relu, asked)
            assert c.narrow_record() is None
            word = _forward_word(c, n, relu, kw, handed_down)
            if asked['narrow64'] == 'mfma':
                assert not measured and c.narrow_record() is None and word == before and word & _capi.KN_FLAG_NARROW64_MFMA
                continue
            assert measured == [(n, relu)] and c.narrow_record()['decided'] == decided
            assert before & _capi.KN_FLAG_NARROW and not before & _capi.KN_FLAG_NARROW_MFMA
            assert bool(word & _capi.KN_FLAG_NARROW_MFMA) == (decided == 'mfma') and word == _launch_word(c, relu, asked)      # once measured, they agree again
            assert (word == before) == (decided == 'exact')
