"""One case per product tuning knob (api.hip kKnobs): the values to run, the shapes at which each value reaches its branch, and how
far a value may move the result.  Read by tests/test_knobs_gpu.py (the sweep on the MI355X) and tests/test_abi_cpu.py (every knob of
the registry has a case here, every listed value is accepted, every value of a value-set knob is listed).

Entry fields:
  kind    'set'       every legal value is listed (0/1 switches, split / chunk counts, bit fields of 2 bits);
          'threshold' values that force the branch on (0 or 1) and off (1 << 30, or the largest accepted value);
          'fields'    a bit field: each field on its own (xcd_mapping).
  bits    'same'      the knob changes placement or priority only: the output is bit for bit the default's;
          'noise'     it changes the fp32 summation order (split counts, chunk counts, kernel choices): within SHAPE_NOISE_PX.
  runs    (values, (pairs, queries), reach[, base knobs]).  reach:
          'changes'        the per-launch profile names (cotr_set_profiling 2: kernel, variant, GEMM configuration) differ from those
                           of the base knobs at that shape;
          'default'        they are the same: the value selects the schedule the default selects (the reason is in `note`);
          ('has', regex)   an in-kernel knob: a launch of the kernel it acts in is in the list;
          'side'           side_stream: profiling turns the side stream off (h->prof), so the eligibility conditions of api.hip
                           forward_impl are asserted instead - one encode pass and one decode pass of B <= encode_chunk pairs,
                           B * Q <= 8192 (cotr_batch_chunks).
          base knobs are set with the knob, for the branches one knob alone cannot reach; the reference output is still the
          default-knob one, the reference launch list the base knobs' one.
Shapes (those of tests/test_parity_gpu.py, and one more): 1 x 1000 the metric configuration; 3 x 333 the unfused middle rows (encoder 1536 rows);
8 x 512 (encoder and decoder on the small-row fused kernels, conv23 / expand); 24 x 100 att_rows / ffn_rows in the encoder, pair-per-XCD
placement, unfused decoder; 17 x 1000 batch_split 16 + 1 (resident attention in the 16-pair encoder pass); 32 x 1 the SparseEngine shape;
65 x 1 the only place encode_chunk 128 differs from 64 (enc_next_chunk: more than 64 pairs).
"""

BIG = 1 << 30

S1, S2, S3, S4, S5, S6, S65 = (1, 1000), (3, 333), (8, 512), (24, 100), (17, 1000), (32, 1), (65, 1)
GEMM_WS = r'cfg4[01]\b'   # the wave-specialised large-tile GEMM (gemm_big.hip gemm_ws_kernel, configurations 40 / 41)

KNOB_CASES = {
    'encode_chunk': dict(kind='threshold', bits='noise', runs=[
        ((1,), S2, 'changes'), ((7,), S5, 'changes'), ((128,), S65, 'changes')],
        note='pairs per encode pass: 3 passes of 1; 7 + 7 + 3 instead of 16 + 1; 65 pairs in one pass instead of 64 + 1'),
    'attention_fusion_max_rows': dict(kind='threshold', bits='noise', runs=[((0,), S1, 'changes'), ((BIG,), S5, 'changes')],
                                      note='0: no fused attention + out_proj anywhere; 1 << 30: the 8192-row encoder pass takes it (8 whole rounds)'),
    'ffn_fusion_max_rows': dict(kind='threshold', bits='noise', runs=[((0,), S1, 'changes'), ((BIG,), S5, 'changes')],
                                note='0: no fused FFN; 1 << 30: 8192 encoder rows fill 2 rounds, and the decoder is no longer cut 16 + 1'),
    'ks3': dict(kind='set', bits='noise', runs=[((0,), S1, 'changes', {'conv_patch': 0}), ((1,), S1, 'default')],
                note='three-stage LDS-DMA k-split (30) for the table\'s 24; conv_patch (31) takes the 3x3 convolutions first, so it is off'),
    'dual_conv': dict(kind='set', bits='noise', runs=[((0,), S1, 'changes'), ((1,), S1, 'default')],
                      note='layer2 / layer3 entry blocks: downsample + conv1 in one launch at one pair'),
    'fused_stem': dict(kind='set', bits='noise', runs=[((0,), S1, 'changes'), ((1,), S1, 'default')],
                       note='stem_pool against conv7x7 + maxpool'),
    'xcd_mapping': dict(kind='fields', bits='same', runs=[
        ((0, 1, 2), S3, ('has', r'^(linear|conv)')),         # bits 0-1: GEMM tiles over XCDs (set_xcd_split)
        ((1 | 4, 1 | 16), S3, ('has', r'^ffn_fused ')),      # bit 2: FFN chunks over XCDs; bit 4: plain stores for the partials
        ((1 | 8,), S3, ('has', r'attention\+oproj')),        # bit 3: heads over XCDs in the attention kernels
        ((1 | 32,), S4, ('has', r'^att_rows enc'))],         # bit 5: att_rows without the pair-per-XCD placement (24 pairs = 3 x 8)
        note='workgroup placement and store flavour only: every tile sums the same products in the same order'),
    'attention_fused_splits': dict(kind='set', bits='noise', runs=[((0, 4), S1, 'default'), ((8, 48, 84), S1, 'changes')],
                                   note='0 means 4; 48 / 84: 4 / 8 key splits in the encoder and 8 / 4 in the decoder'),
    'conv_patch': dict(kind='set', bits='noise', runs=[((0,), S1, 'changes'), ((1,), S1, 'default')],
                       note='3x3 stride-1 convolutions over 256 channels with the input patch loaded once (configuration 31)'),
    'pos_table_min_rows': dict(kind='threshold', bits='noise', runs=[((0,), S1, 'changes'), ((BIG,), S4, 'changes')],
                               note='the encoder in-projections take the pos table (+table) instead of the x + pos prologue (+pos); '
                                    '1 << 30 also moves the decoder K/V projection to the prologue'),
    'attention_wide_occupancy': dict(kind='set', bits='noise', runs=[((2,), S2, ('has', r'attention enc wide2'), {'attention_wide_min_rows': 0}),
                                                                     ((3,), S2, ('has', r'attention enc wide3'), {'attention_wide_min_rows': 0})],
                                     note='the 64-query kernel\'s occupancy template; no default shape runs that kernel, so it is forced'),
    'attention_wide_min_rows': dict(kind='threshold', bits='noise', runs=[((0,), S2, 'changes'),
                                                                         ((BIG,), S5, 'changes', {'attention_resident': 0})],
                                    note='0: the 1536-row encoder attention on the 64-query kernel; 1 << 30: the 16-pair pass back on 4 splits'),
    'attention_splits': dict(kind='set', bits='noise', runs=[((0,), S2, 'default'), ((1, 2, 8, 16), S2, 'changes'), ((4,), S5, 'changes')],
                             note='0 = automatic (4 splits where neither the resident nor the 64-query kernel applies: 3 x 333 encoder); '
                                  '4 forces the split kernel where the resident one runs'),
    'conv1x1_dense': dict(kind='set', bits='noise', runs=[((0,), S1, 'changes'), ((1,), S1, 'default')],
                          note='1x1 stride-1 convolutions on the dense instantiation (dense) or the convolution one'),
    'ws_flags': dict(kind='set', bits='same', runs=[((0, 1, 2, 3), S2, ('has', GEMM_WS))],
                     note='s_setprio of the loader / MFMA wavefronts of the wave-specialised GEMM only'),
    'bottleneck_max_pairs': dict(kind='threshold', bits='noise', runs=[((0,), S1, 'changes'), ((BIG,), S3, 'changes')],
                                 note='layer1 bottlenecks as one launch: off at one pair; on at 8 pairs (instead of conv23 / expand)'),
    'attention_resident': dict(kind='set', bits='noise', runs=[((0,), S5, 'changes'), ((1,), S5, ('has', r'attention enc res'))],
                               note='the resident-K/V attention kernel in the 16-pair encoder pass; 0: the 64-query kernel'),
    'att_rows_min_rows': dict(kind='threshold', bits='noise', runs=[((0,), S2, 'changes', {'rows_min_fill': 0}), ((BIG,), S4, 'changes')],
                              note='alone, 0 is the default: no att_rows grid below 8192 rows fills 75 % of a round, hence rows_min_fill 0'),
    'ffn_rows_min_rows': dict(kind='threshold', bits='noise', runs=[((0,), S2, 'changes', {'rows_min_fill': 0}), ((BIG,), S4, 'changes')],
                              note='alone, 0 is the default: no ffn_rows grid below 8192 rows fills 75 % of a round, hence rows_min_fill 0'),
    'conv23_min_pairs': dict(kind='threshold', bits='noise', runs=[((1,), S2, 'changes', {'bottleneck_max_pairs': 0}), ((BIG,), S3, 'changes')],
                             note='conv23 runs above bottleneck_max_pairs only, so its low end needs the bottleneck launch off'),
    'conv23m_min_pairs': dict(kind='threshold', bits='noise', runs=[((1,), S3, 'changes'), ((BIG,), S6, 'changes')],
                              note='layer2 conv2 -> conv3 in one launch at 8 pairs (one workgroup per CU and less) / off at 32'),
    'expand_min_rows': dict(kind='threshold', bits='noise', runs=[((0,), S1, 'changes', {'bottleneck_max_pairs': 0}), ((BIG,), S3, 'changes')],
                            note='layer1 block 0 downsample + conv1 in one launch; at one pair only once the bottleneck launch is off'),
    'rows_min_fill': dict(kind='threshold', bits='noise', runs=[((0,), S5, 'changes'), ((100,), S4, 'changes')],
                          note='0: att_rows / ffn_rows take the half-round 16-pair encoder pass; 100: not the 3/4-round 24-pair one'),
    'side_stream': dict(kind='set', bits='noise', runs=[((0,), S1, 'default'), ((1, 2, 3), S1, 'side')],
                        note='bit 0 moves the query encoding to a second stream (same launch); bit 1 runs the K/V projection as two '
                             'GEMMs - layer 0\'s 512 columns, then the other 2560 beside it - whose configurations are picked per shape'),
    'ffn_fused_max_chunks': dict(kind='set', bits='noise', runs=[((2, 4, 8), S1, 'changes'), ((16,), S1, 'default')],
                                 note='hidden-unit chunks (partial outputs) of the fused FFN at 1000 rows'),
    'batch_split': dict(kind='set', bits='noise', runs=[((0,), S5, 'changes'), ((1,), S5, 'default')],
                        note='17 pairs: one pass instead of 16 + 1 (encode and decode)'),
}

# product knobs without a case here, and why
KNOB_EXCLUDED = {
    'train_attention_form': 'training step only (attention backward form); tests/test_train_ops_gpu.py runs forms 0-3',
}


def case_values(name):
    """every value a case runs, in table order"""
    out = []
    for run in KNOB_CASES[name]['runs']:
        out += [v for v in run[0] if v not in out]
    return out


def case_runs():
    """(knob, value, shape, reach, base) for every run of the table"""
    for name, case in KNOB_CASES.items():
        for run in case['runs']:
            values, shape, reach = run[:3]
            base = run[3] if len(run) > 3 else {}
            for v in values:
                yield name, v, shape, reach, base
