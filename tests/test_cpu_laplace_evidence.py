"""The Laplace log evidence without a GPU: the C-ABI declaration of pgpfa_get_log_evidence and its info key, the binding, the module switch and
the keywords of engine.PPGPFAfit and util.crossValidation; the numbers are tests/test_gpu_laplace_evidence.py's."""
import inspect
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope='module')
def built():
    import __graft_entry__ as ge
    ge.build()
    import funs
    return funs


def test_header_binding_and_library_agree_on_the_new_entry_point(built):
    from funs import _hip
    lib = _hip.load_library()
    header = open(os.path.join(ROOT, 'include', 'pgpfa.h')).read()
    assert re.search(r'int\s+pgpfa_get_log_evidence\s*\(\s*pgpfa_ctx\s*\*\s*ctx\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*idx\s*,\s*double\s*\*\s*out', header)
    assert 'pgpfa_get_log_evidence' in _hip.EXPORTED_SYMBOLS and hasattr(lib, 'pgpfa_get_log_evidence')
    assert '"last_log_evidence_sum"' in header and '"laplace_evidence"' in header
    # the header cites the reference lines the quantity is built from and states the normalisation
    doc = header[:header.index('int pgpfa_get_log_evidence')].rsplit('/*', 1)[1]
    for cite in ('inference.py:12-32', 'inference.py:50-65', 'inference.py:130-131', 'log y!'):
        assert cite in doc, cite
    assert hasattr(_hip.Context, 'log_evidence')
    assert list(inspect.signature(_hip.Context.log_evidence).parameters) == ['self', 'idx']


def test_module_switch_and_keywords(built):
    from funs import engine, inference, util
    assert inference.LAPLACE_EVIDENCE is False
    par = inspect.signature(engine.PPGPFAfit.__init__).parameters
    names = list(par)
    assert names[-4:] == ['quiet', 'onlineWarmStart', 'trackEvidence', 'emTol']
    for name, default in (('trackEvidence', False), ('emTol', None)):
        assert par[name].kind is inspect.Parameter.KEYWORD_ONLY and par[name].default is default
    assert inspect.signature(util.crossValidation.__init__).parameters['score'].default == 'loo'
    # laplace()'s own signature and return are the reference's: nothing added there
    assert list(inspect.signature(inference.laplace).parameters) == ['experiment', 'params', 'prevOptimRes', 'returnOptimRes', 'verbose', 'optimMethod']


def test_keyword_errors_come_before_any_device_work(built):
    from funs import engine, util
    with pytest.raises(ValueError, match="emTol needs EMmode='Batch'"):
        engine.PPGPFAfit(None, initParams=None, EMmode='Online', emTol=1e-3)
    with pytest.raises(ValueError, match='emTol must be a positive float'):
        engine.PPGPFAfit(None, initParams=None, EMmode='Batch', emTol=0.0)
    with pytest.raises(ValueError, match="score must be 'loo' or 'evidence'"):
        util.crossValidation(None, score='bic')
    with pytest.raises(ValueError, match="needs inferenceMethod='laplace'"):
        util.crossValidation(None, inferenceMethod='variational', score='evidence')
