"""The code-generation checks of tests/test_codegen.py (tools/codegen_report.py) on every hyper-connection pre-norm GEMM instantiation in
the built library: no scratch between the first and last MFMA, no VGPR spills, no waterfall loop at the K loop, no landing or SGPR -> VMEM
hazards."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KERNELS = [f'dg_hc_prenorm_gemm_kernel<{ms},{ns}>' for ms in (1, 8) for ns in (1, 2)]


def test_hc_prenorm_kernels_codegen():
    spec = importlib.util.spec_from_file_location('codegen_report', os.path.join(ROOT, 'tools', 'codegen_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = [r for r in mod.report() if r['kernel'].startswith('dg_hc_prenorm_gemm_kernel<')]
    assert sorted(r['kernel'] for r in rows) == sorted(KERNELS)
    for r in rows:
        name = r['kernel']
        assert r['mfma_range_instructions'] > 0, name
        assert r['scratch_in_mfma_range'] == 0, name
        assert r.get('vgpr_spill_count', 0) == 0, name
        assert r['waterfalls_at_k_loop'] == 0, name
        assert not r['landing_touches'], name
        assert not r['sgpr_vmem_hazards'], name
