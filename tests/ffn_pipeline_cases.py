"""Cases shared by tests/test_ffn_pipeline_gpu.py and the generator of its fixture (tests/golden/make_ffn_pipeline_fixtures.py)."""
EDGE_ROWS = [64, 65, 97]      # two and three 32-row tiles, the last one full, holding one row, holding one row behind two full tiles
EDGE_CHUNKS = [16, 8, 2]      # knob ffn_fused_max_chunks -> 2, 4 and 16 steps of 32 hidden units per workgroup
