"""The code-generation checks of tests/test_codegen.py (tools/codegen_report.py) on every BF16 kernel instantiation in the built library:
no scratch between the first and last MFMA, no waterfall loop at the K loop, no landing or SGPR -> VMEM hazards."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bf16_kernels_codegen():
    spec = importlib.util.spec_from_file_location('codegen_report', os.path.join(ROOT, 'tools', 'codegen_report.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = [r for r in mod.report() if r['kernel'].startswith('dg_bf16_gemm_')]
    assert sorted(r['kernel'] for r in rows) == sorted(['dg_bf16_gemm_kernel<256,256,2,4,2,0>', 'dg_bf16_gemm_kernel<128,256,2,4,3,0>',
                                                        'dg_bf16_gemm_kernel<64,32,4,1,8,0>', 'dg_bf16_gemm_kernel<64,32,4,1,8,1>'])
    for r in rows:
        name = r['kernel']
        assert r['mfma_range_instructions'] > 0, name
        assert r['scratch_in_mfma_range'] == 0, name
        assert r.get('vgpr_spill_count', 0) == 0, name
        assert r['waterfalls_at_k_loop'] == 0, name
        assert not r['landing_touches'], name
        assert not r['landing_branches_in_mfma_range'], name
        assert not r['sgpr_vmem_hazards'], name
