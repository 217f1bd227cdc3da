"""The code-generation checks of tests/test_codegen.py (tools/codegen_report.py) on every MQA logits kernel instantiation in the built
library: no scratch between the first and last MFMA, no VGPR spills, no waterfall loop at the KV loop, no landing or SGPR -> VMEM hazards."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DENSE = [f'dg_mqa_logits_kernel<{h},{d}>' for h in (8, 16, 32, 64) for d in (32, 64, 128)]
PAGED = [f'dg_paged_mqa_logits_kernel<{h},{d},{mt}>' for h in (8, 16, 32, 64) for d in (32, 64, 128) for mt in (1, 2, 4, 8) if mt * 16 >= h]


def test_mqa_logits_kernels_codegen():
    spec = importlib.util.spec_from_file_location('codegen_report', os.path.join(ROOT, 'tools', 'codegen_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = [r for r in mod.report() if r['kernel'].startswith(('dg_mqa_logits_kernel<', 'dg_paged_mqa_logits_kernel<'))]
    assert sorted(r['kernel'] for r in rows) == sorted(DENSE + PAGED)
    for r in rows:
        name = r['kernel']
        assert r['mfma_range_instructions'] > 0, name
        assert r['scratch_in_mfma_range'] == 0, name
        assert r.get('vgpr_spill_count', 0) == 0, name
        assert r['waterfalls_at_k_loop'] == 0, name
        assert not r['landing_touches'], name
        assert not r['sgpr_vmem_hazards'], name
