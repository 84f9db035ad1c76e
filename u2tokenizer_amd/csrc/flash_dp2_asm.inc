// clang-format off
#define FLASH_DP2_ASM_TEXT \
  "v_add_u32 v70, %[lds], %[ab0]\n" \
  "v_xor_b32 v71, 32, v70\n" \
  "v_xor_b32 v72, 64, v70\n" \
  "v_xor_b32 v73, 96, v70\n" \
  "global_load_dwordx4 v[36:39], %[qa0], off offset:0\n" \
  "global_load_dwordx4 v[40:43], %[qa0], off offset:32\n" \
  "global_load_dwordx4 v[44:47], %[qa0], off offset:64\n" \
  "global_load_dwordx4 v[48:51], %[qa0], off offset:96\n" \
  "global_load_dwordx4 v[52:55], %[qa1], off offset:0\n" \
  "global_load_dwordx4 v[56:59], %[qa1], off offset:32\n" \
  "global_load_dwordx4 v[60:63], %[qa1], off offset:64\n" \
  "global_load_dwordx4 v[64:67], %[qa1], off offset:96\n" \
  "global_load_dwordx2 v[186:187], %[vxa], off offset:0\n" \
  "global_load_dwordx2 v[188:189], %[vxa], off offset:16\n" \
  "global_load_dwordx2 v[190:191], %[vxa], off offset:32\n" \
  "global_load_dwordx2 v[192:193], %[vxa], off offset:48\n" \
  "global_load_dwordx2 v[194:195], %[vxa], off offset:64\n" \
  "global_load_dwordx2 v[196:197], %[vxa], off offset:80\n" \
  "global_load_dwordx2 v[198:199], %[vxa], off offset:96\n" \
  "global_load_dwordx2 v[200:201], %[vxa], off offset:112\n" \
  "global_load_dwordx4 v[154:157], %[kxa], off offset:0\n" \
  "global_load_dwordx4 v[158:161], %[kxa], off offset:32\n" \
  "global_load_dwordx4 v[162:165], %[kxa], off offset:64\n" \
  "global_load_dwordx4 v[166:169], %[kxa], off offset:96\n" \
  "s_mov_b32 s36, 0\n" \
  "s_mov_b32 s37, 0\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 m0, %[dma_base], 0\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 1024\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 8192\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 9216\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "s_add_u32 s37, s37, 1\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 m0, %[dma_base], 16384\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 17408\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 24576\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 25600\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "s_add_u32 s37, s37, 1\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 m0, %[dma_base], 32768\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 33792\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 40960\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 41984\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "s_add_u32 s37, s37, 1\n" \
  "v_mov_b32 v210, 0xff800000\n" \
  "v_mov_b32 v211, 0xff800000\n" \
  "s_cmp_eq_u32 %[xflag], 0\n" \
  "s_cbranch_scc1 .Lfd2_nox_%=\n" \
  "s_waitcnt vmcnt(12)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[154:157], v[36:39], 0\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[158:161], v[40:43], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[162:165], v[44:47], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[166:169], v[48:51], v[138:153]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_mov_b32 v210, v138\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[154:157], v[52:55], 0\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[158:161], v[56:59], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[162:165], v[60:63], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[166:169], v[64:67], v[138:153]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_mov_b32 v211, v138\n" \
  ".Lfd2_nox_%=:\n" \
  "s_waitcnt vmcnt(8)\n" \
  "s_barrier\n" \
  "s_mov_b32 s38, %[seq]\n" \
  "ds_read_b128 v[218:221], v70 offset:0\n" \
  "ds_read_b128 v[222:225], v71 offset:0\n" \
  "ds_read_b128 v[226:229], v72 offset:0\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], 0\n" \
  "ds_read_b128 v[230:233], v73 offset:0\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[222:225], v[40:43], v[138:153]\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[44:47], v[138:153]\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[230:233], v[48:51], v[138:153]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask1_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc2_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret2_%=-.Lfd2_pc2_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret2_%=:\n" \
  ".Lfd2_nomask1_%=:\n" \
  "v_max3_f32 v252, v138, v139, v140\n" \
  "v_max3_f32 v253, v141, v142, v143\n" \
  "v_max3_f32 v255, v144, v145, v146\n" \
  "v_max3_f32 v69, v147, v148, v149\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v150, v151, v152\n" \
  "v_max3_f32 v69, v69, v253, v153\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, v252, v210\n" \
  "v_mov_b32 %[mr0], v252\n" \
  "v_sub_f32 v255, v210, v252\n" \
  "v_exp_f32 v255, v255\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr0], 0.5, v255\n" \
  "v_lshlrev_b32 v253, 16, v186\n" \
  "v_mul_f32 v74, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v186\n" \
  "v_mul_f32 v75, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v187\n" \
  "v_mul_f32 v76, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v187\n" \
  "v_mul_f32 v77, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v188\n" \
  "v_mul_f32 v78, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v188\n" \
  "v_mul_f32 v79, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v189\n" \
  "v_mul_f32 v80, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v189\n" \
  "v_mul_f32 v81, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v190\n" \
  "v_mul_f32 v82, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v190\n" \
  "v_mul_f32 v83, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v191\n" \
  "v_mul_f32 v84, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v191\n" \
  "v_mul_f32 v85, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v192\n" \
  "v_mul_f32 v86, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v192\n" \
  "v_mul_f32 v87, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v193\n" \
  "v_mul_f32 v88, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v193\n" \
  "v_mul_f32 v89, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v194\n" \
  "v_mul_f32 v90, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v194\n" \
  "v_mul_f32 v91, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v195\n" \
  "v_mul_f32 v92, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v195\n" \
  "v_mul_f32 v93, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v196\n" \
  "v_mul_f32 v94, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v196\n" \
  "v_mul_f32 v95, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v197\n" \
  "v_mul_f32 v96, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v197\n" \
  "v_mul_f32 v97, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v198\n" \
  "v_mul_f32 v98, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v198\n" \
  "v_mul_f32 v99, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v199\n" \
  "v_mul_f32 v100, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v199\n" \
  "v_mul_f32 v101, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v200\n" \
  "v_mul_f32 v102, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v200\n" \
  "v_mul_f32 v103, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v201\n" \
  "v_mul_f32 v104, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v201\n" \
  "v_mul_f32 v105, v255, v253\n" \
  "v_sub_f32 v170, 0, v252\n" \
  "v_sub_f32 v171, 0, v252\n" \
  "v_sub_f32 v172, 0, v252\n" \
  "v_sub_f32 v173, 0, v252\n" \
  "v_sub_f32 v174, 0, v252\n" \
  "v_sub_f32 v175, 0, v252\n" \
  "v_sub_f32 v176, 0, v252\n" \
  "v_sub_f32 v177, 0, v252\n" \
  "v_sub_f32 v178, 0, v252\n" \
  "v_sub_f32 v179, 0, v252\n" \
  "v_sub_f32 v180, 0, v252\n" \
  "v_sub_f32 v181, 0, v252\n" \
  "v_sub_f32 v182, 0, v252\n" \
  "v_sub_f32 v183, 0, v252\n" \
  "v_sub_f32 v184, 0, v252\n" \
  "v_sub_f32 v185, 0, v252\n" \
  "v_sub_f32 v138, v138, v252\n" \
  "v_sub_f32 v139, v139, v252\n" \
  "v_sub_f32 v140, v140, v252\n" \
  "v_sub_f32 v141, v141, v252\n" \
  "v_sub_f32 v142, v142, v252\n" \
  "v_sub_f32 v143, v143, v252\n" \
  "v_sub_f32 v144, v144, v252\n" \
  "v_sub_f32 v145, v145, v252\n" \
  "v_sub_f32 v146, v146, v252\n" \
  "v_sub_f32 v147, v147, v252\n" \
  "v_sub_f32 v148, v148, v252\n" \
  "v_sub_f32 v149, v149, v252\n" \
  "v_sub_f32 v150, v150, v252\n" \
  "v_sub_f32 v151, v151, v252\n" \
  "v_sub_f32 v152, v152, v252\n" \
  "v_sub_f32 v153, v153, v252\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], 0\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[222:225], v[56:59], v[154:169]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[230:233], v[64:67], v[154:169]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:4096\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:8192\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:4096\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok3_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc4_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret4_%=-.Lfd2_pc4_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret4_%=:\n" \
  ".Lfd2_ok3_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask5_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc6_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret6_%=-.Lfd2_pc6_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret6_%=:\n" \
  ".Lfd2_nomask5_%=:\n" \
  "v_max3_f32 v252, v154, v155, v156\n" \
  "v_max3_f32 v253, v157, v158, v159\n" \
  "v_max3_f32 v255, v160, v161, v162\n" \
  "v_max3_f32 v69, v163, v164, v165\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v166, v167, v168\n" \
  "v_max3_f32 v69, v69, v253, v169\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, v252, v211\n" \
  "v_mov_b32 %[mr1], v252\n" \
  "v_sub_f32 v255, v211, v252\n" \
  "v_exp_f32 v255, v255\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr1], 0.5, v255\n" \
  "v_lshlrev_b32 v253, 16, v186\n" \
  "v_mul_f32 v106, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v186\n" \
  "v_mul_f32 v107, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v187\n" \
  "v_mul_f32 v108, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v187\n" \
  "v_mul_f32 v109, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v188\n" \
  "v_mul_f32 v110, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v188\n" \
  "v_mul_f32 v111, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v189\n" \
  "v_mul_f32 v112, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v189\n" \
  "v_mul_f32 v113, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v190\n" \
  "v_mul_f32 v114, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v190\n" \
  "v_mul_f32 v115, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v191\n" \
  "v_mul_f32 v116, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v191\n" \
  "v_mul_f32 v117, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v192\n" \
  "v_mul_f32 v118, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v192\n" \
  "v_mul_f32 v119, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v193\n" \
  "v_mul_f32 v120, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v193\n" \
  "v_mul_f32 v121, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v194\n" \
  "v_mul_f32 v122, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v194\n" \
  "v_mul_f32 v123, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v195\n" \
  "v_mul_f32 v124, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v195\n" \
  "v_mul_f32 v125, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v196\n" \
  "v_mul_f32 v126, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v196\n" \
  "v_mul_f32 v127, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v197\n" \
  "v_mul_f32 v128, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v197\n" \
  "v_mul_f32 v129, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v198\n" \
  "v_mul_f32 v130, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v198\n" \
  "v_mul_f32 v131, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v199\n" \
  "v_mul_f32 v132, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v199\n" \
  "v_mul_f32 v133, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v200\n" \
  "v_mul_f32 v134, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v200\n" \
  "v_mul_f32 v135, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v201\n" \
  "v_mul_f32 v136, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v201\n" \
  "v_mul_f32 v137, v255, v253\n" \
  "v_sub_f32 v186, 0, v252\n" \
  "v_sub_f32 v187, 0, v252\n" \
  "v_sub_f32 v188, 0, v252\n" \
  "v_sub_f32 v189, 0, v252\n" \
  "v_sub_f32 v190, 0, v252\n" \
  "v_sub_f32 v191, 0, v252\n" \
  "v_sub_f32 v192, 0, v252\n" \
  "v_sub_f32 v193, 0, v252\n" \
  "v_sub_f32 v194, 0, v252\n" \
  "v_sub_f32 v195, 0, v252\n" \
  "v_sub_f32 v196, 0, v252\n" \
  "v_sub_f32 v197, 0, v252\n" \
  "v_sub_f32 v198, 0, v252\n" \
  "v_sub_f32 v199, 0, v252\n" \
  "v_sub_f32 v200, 0, v252\n" \
  "v_sub_f32 v201, 0, v252\n" \
  "v_sub_f32 v154, v154, v252\n" \
  "v_sub_f32 v155, v155, v252\n" \
  "v_sub_f32 v156, v156, v252\n" \
  "v_sub_f32 v157, v157, v252\n" \
  "v_sub_f32 v158, v158, v252\n" \
  "v_sub_f32 v159, v159, v252\n" \
  "v_sub_f32 v160, v160, v252\n" \
  "v_sub_f32 v161, v161, v252\n" \
  "v_sub_f32 v162, v162, v252\n" \
  "v_sub_f32 v163, v163, v252\n" \
  "v_sub_f32 v164, v164, v252\n" \
  "v_sub_f32 v165, v165, v252\n" \
  "v_sub_f32 v166, v166, v252\n" \
  "v_sub_f32 v167, v167, v252\n" \
  "v_sub_f32 v168, v168, v252\n" \
  "v_sub_f32 v169, v169, v252\n" \
  ".p2align 6\n" \
  ".Lfd2_loop_%=:\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:12288\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:4096\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:8192\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:4096\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:12288\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok7_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc8_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret8_%=-.Lfd2_pc8_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret8_%=:\n" \
  ".Lfd2_ok7_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask9_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc10_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret10_%=-.Lfd2_pc10_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret10_%=:\n" \
  ".Lfd2_nomask9_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok11_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc12_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret12_%=-.Lfd2_pc12_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret12_%=:\n" \
  ".Lfd2_ok11_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask13_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc14_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret14_%=-.Lfd2_pc14_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret14_%=:\n" \
  ".Lfd2_nomask13_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 8192\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:16384\n" \
  "ds_read_b128 v[222:225], v72 offset:8192\n" \
  "ds_read_b128 v[226:229], v71 offset:16384\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:12288\n" \
  "s_add_u32 m0, %[dma_base], 49152\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:16384\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:8192\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 50176\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:16384\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:12288\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 57344\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 58368\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok15_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc16_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret16_%=-.Lfd2_pc16_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret16_%=:\n" \
  ".Lfd2_ok15_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask17_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc18_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret18_%=-.Lfd2_pc18_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret18_%=:\n" \
  ".Lfd2_nomask17_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:20480\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:24576\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:20480\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok19_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc20_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret20_%=-.Lfd2_pc20_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret20_%=:\n" \
  ".Lfd2_ok19_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask21_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc22_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret22_%=-.Lfd2_pc22_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret22_%=:\n" \
  ".Lfd2_nomask21_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:28672\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:20480\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:24576\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:20480\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:28672\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok23_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc24_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret24_%=-.Lfd2_pc24_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret24_%=:\n" \
  ".Lfd2_ok23_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask25_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc26_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret26_%=-.Lfd2_pc26_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret26_%=:\n" \
  ".Lfd2_nomask25_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok27_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc28_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret28_%=-.Lfd2_pc28_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret28_%=:\n" \
  ".Lfd2_ok27_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask29_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc30_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret30_%=-.Lfd2_pc30_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret30_%=:\n" \
  ".Lfd2_nomask29_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 24576\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:32768\n" \
  "ds_read_b128 v[222:225], v72 offset:24576\n" \
  "ds_read_b128 v[226:229], v71 offset:32768\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:28672\n" \
  "s_add_u32 m0, %[dma_base], 0\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:32768\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:24576\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 1024\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:32768\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:28672\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 8192\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 9216\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok31_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc32_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret32_%=-.Lfd2_pc32_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret32_%=:\n" \
  ".Lfd2_ok31_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask33_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc34_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret34_%=-.Lfd2_pc34_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret34_%=:\n" \
  ".Lfd2_nomask33_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:36864\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:40960\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:36864\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok35_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc36_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret36_%=-.Lfd2_pc36_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret36_%=:\n" \
  ".Lfd2_ok35_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask37_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc38_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret38_%=-.Lfd2_pc38_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret38_%=:\n" \
  ".Lfd2_nomask37_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:45056\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:36864\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:40960\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:36864\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:45056\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok39_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc40_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret40_%=-.Lfd2_pc40_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret40_%=:\n" \
  ".Lfd2_ok39_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask41_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc42_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret42_%=-.Lfd2_pc42_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret42_%=:\n" \
  ".Lfd2_nomask41_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok43_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc44_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret44_%=-.Lfd2_pc44_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret44_%=:\n" \
  ".Lfd2_ok43_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask45_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc46_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret46_%=-.Lfd2_pc46_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret46_%=:\n" \
  ".Lfd2_nomask45_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 40960\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:49152\n" \
  "ds_read_b128 v[222:225], v72 offset:40960\n" \
  "ds_read_b128 v[226:229], v71 offset:49152\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:45056\n" \
  "s_add_u32 m0, %[dma_base], 16384\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:49152\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:40960\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 17408\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:49152\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:45056\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 24576\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 25600\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok47_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc48_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret48_%=-.Lfd2_pc48_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret48_%=:\n" \
  ".Lfd2_ok47_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask49_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc50_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret50_%=-.Lfd2_pc50_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret50_%=:\n" \
  ".Lfd2_nomask49_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:53248\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:57344\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:53248\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok51_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc52_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret52_%=-.Lfd2_pc52_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret52_%=:\n" \
  ".Lfd2_ok51_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask53_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc54_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret54_%=-.Lfd2_pc54_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret54_%=:\n" \
  ".Lfd2_nomask53_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:61440\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:53248\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:57344\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:53248\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:61440\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok55_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc56_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret56_%=-.Lfd2_pc56_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret56_%=:\n" \
  ".Lfd2_ok55_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask57_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc58_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret58_%=-.Lfd2_pc58_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret58_%=:\n" \
  ".Lfd2_nomask57_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok59_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc60_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret60_%=-.Lfd2_pc60_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret60_%=:\n" \
  ".Lfd2_ok59_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask61_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc62_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret62_%=-.Lfd2_pc62_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret62_%=:\n" \
  ".Lfd2_nomask61_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 57344\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:0\n" \
  "ds_read_b128 v[222:225], v72 offset:57344\n" \
  "ds_read_b128 v[226:229], v71 offset:0\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:61440\n" \
  "s_add_u32 m0, %[dma_base], 32768\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:57344\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 33792\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:61440\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 40960\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 41984\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok63_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc64_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret64_%=-.Lfd2_pc64_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret64_%=:\n" \
  ".Lfd2_ok63_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask65_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc66_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret66_%=-.Lfd2_pc66_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret66_%=:\n" \
  ".Lfd2_nomask65_%=:\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:4096\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:8192\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:4096\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok67_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc68_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret68_%=-.Lfd2_pc68_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret68_%=:\n" \
  ".Lfd2_ok67_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask69_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc70_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret70_%=-.Lfd2_pc70_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret70_%=:\n" \
  ".Lfd2_nomask69_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_branch .Lfd2_loop_%=\n" \
  ".Lfd2_epi_%=:\n" \
  "v_add_u32 v69, s43, v72\n" \
  "ds_read_b128 v[218:221], v69 offset:0\n" \
  "v_add_u32 v69, s43, v72\n" \
  "ds_read_b128 v[222:225], v69 offset:4096\n" \
  "v_add_u32 v69, s43, v73\n" \
  "ds_read_b128 v[226:229], v69 offset:0\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[218:221], v[202:205], v[74:89]\n" \
  "v_add_u32 v69, s43, v73\n" \
  "ds_read_b128 v[230:233], v69 offset:4096\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[222:225], v[202:205], v[90:105]\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[226:229], v[206:209], v[74:89]\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok71_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc72_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret72_%=-.Lfd2_pc72_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret72_%=:\n" \
  ".Lfd2_ok71_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[218:221], v[210:213], v[106:121]\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[222:225], v[210:213], v[122:137]\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[226:229], v[214:217], v[106:121]\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[214:217], v[122:137]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n" \
  "s_barrier\n" \
  "ds_write_b128 %[dump], v[74:77] offset:0\n" \
  "ds_write_b128 %[dump], v[78:81] offset:1024\n" \
  "ds_write_b128 %[dump], v[82:85] offset:2048\n" \
  "ds_write_b128 %[dump], v[86:89] offset:3072\n" \
  "ds_write_b128 %[dump], v[90:93] offset:4096\n" \
  "ds_write_b128 %[dump], v[94:97] offset:5120\n" \
  "ds_write_b128 %[dump], v[98:101] offset:6144\n" \
  "ds_write_b128 %[dump], v[102:105] offset:7168\n" \
  "ds_write_b128 %[dump], v[106:109] offset:8192\n" \
  "ds_write_b128 %[dump], v[110:113] offset:9216\n" \
  "ds_write_b128 %[dump], v[114:117] offset:10240\n" \
  "ds_write_b128 %[dump], v[118:121] offset:11264\n" \
  "ds_write_b128 %[dump], v[122:125] offset:12288\n" \
  "ds_write_b128 %[dump], v[126:129] offset:13312\n" \
  "ds_write_b128 %[dump], v[130:133] offset:14336\n" \
  "ds_write_b128 %[dump], v[134:137] offset:15360\n" \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n" \
  "v_mbcnt_lo_u32_b32 %[lid], -1, 0\n" \
  "v_mbcnt_hi_u32_b32 %[lid], -1, %[lid]\n" \
  "s_branch .Lfd2_end_%=\n" \
  ".Lfd2_slow0_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_max3_f32 v252, v138, v139, v140\n" \
  "v_max3_f32 v253, v141, v142, v143\n" \
  "v_max3_f32 v255, v144, v145, v146\n" \
  "v_max3_f32 v69, v147, v148, v149\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v150, v151, v152\n" \
  "v_max3_f32 v69, v69, v253, v153\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, 0, v252\n" \
  "v_sub_f32 v255, 0, v252\n" \
  "v_exp_f32 v255, v255\n" \
  "v_add_f32 %[mr0], %[mr0], v252\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr0], %[lr0], v255\n" \
  "v_mul_f32 v74, v74, v255\n" \
  "v_mul_f32 v75, v75, v255\n" \
  "v_mul_f32 v76, v76, v255\n" \
  "v_mul_f32 v77, v77, v255\n" \
  "v_mul_f32 v78, v78, v255\n" \
  "v_mul_f32 v79, v79, v255\n" \
  "v_mul_f32 v80, v80, v255\n" \
  "v_mul_f32 v81, v81, v255\n" \
  "v_mul_f32 v82, v82, v255\n" \
  "v_mul_f32 v83, v83, v255\n" \
  "v_mul_f32 v84, v84, v255\n" \
  "v_mul_f32 v85, v85, v255\n" \
  "v_mul_f32 v86, v86, v255\n" \
  "v_mul_f32 v87, v87, v255\n" \
  "v_mul_f32 v88, v88, v255\n" \
  "v_mul_f32 v89, v89, v255\n" \
  "v_mul_f32 v90, v90, v255\n" \
  "v_mul_f32 v91, v91, v255\n" \
  "v_mul_f32 v92, v92, v255\n" \
  "v_mul_f32 v93, v93, v255\n" \
  "v_mul_f32 v94, v94, v255\n" \
  "v_mul_f32 v95, v95, v255\n" \
  "v_mul_f32 v96, v96, v255\n" \
  "v_mul_f32 v97, v97, v255\n" \
  "v_mul_f32 v98, v98, v255\n" \
  "v_mul_f32 v99, v99, v255\n" \
  "v_mul_f32 v100, v100, v255\n" \
  "v_mul_f32 v101, v101, v255\n" \
  "v_mul_f32 v102, v102, v255\n" \
  "v_mul_f32 v103, v103, v255\n" \
  "v_mul_f32 v104, v104, v255\n" \
  "v_mul_f32 v105, v105, v255\n" \
  "v_sub_f32 v170, v170, v252\n" \
  "v_sub_f32 v171, v171, v252\n" \
  "v_sub_f32 v172, v172, v252\n" \
  "v_sub_f32 v173, v173, v252\n" \
  "v_sub_f32 v174, v174, v252\n" \
  "v_sub_f32 v175, v175, v252\n" \
  "v_sub_f32 v176, v176, v252\n" \
  "v_sub_f32 v177, v177, v252\n" \
  "v_sub_f32 v178, v178, v252\n" \
  "v_sub_f32 v179, v179, v252\n" \
  "v_sub_f32 v180, v180, v252\n" \
  "v_sub_f32 v181, v181, v252\n" \
  "v_sub_f32 v182, v182, v252\n" \
  "v_sub_f32 v183, v183, v252\n" \
  "v_sub_f32 v184, v184, v252\n" \
  "v_sub_f32 v185, v185, v252\n" \
  "v_sub_f32 v138, v138, v252\n" \
  "v_sub_f32 v139, v139, v252\n" \
  "v_sub_f32 v140, v140, v252\n" \
  "v_sub_f32 v141, v141, v252\n" \
  "v_sub_f32 v142, v142, v252\n" \
  "v_sub_f32 v143, v143, v252\n" \
  "v_sub_f32 v144, v144, v252\n" \
  "v_sub_f32 v145, v145, v252\n" \
  "v_sub_f32 v146, v146, v252\n" \
  "v_sub_f32 v147, v147, v252\n" \
  "v_sub_f32 v148, v148, v252\n" \
  "v_sub_f32 v149, v149, v252\n" \
  "v_sub_f32 v150, v150, v252\n" \
  "v_sub_f32 v151, v151, v252\n" \
  "v_sub_f32 v152, v152, v252\n" \
  "v_sub_f32 v153, v153, v252\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_add_f32 v254, v250, v251\n" \
  "v_exp_f32 v250, v140\n" \
  "v_exp_f32 v251, v141\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v203, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v144\n" \
  "v_exp_f32 v251, v145\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v205, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v148\n" \
  "v_exp_f32 v251, v149\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v207, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v152\n" \
  "v_exp_f32 v251, v153\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v209, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_slow1_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_max3_f32 v252, v154, v155, v156\n" \
  "v_max3_f32 v253, v157, v158, v159\n" \
  "v_max3_f32 v255, v160, v161, v162\n" \
  "v_max3_f32 v69, v163, v164, v165\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v166, v167, v168\n" \
  "v_max3_f32 v69, v69, v253, v169\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, 0, v252\n" \
  "v_sub_f32 v255, 0, v252\n" \
  "v_exp_f32 v255, v255\n" \
  "v_add_f32 %[mr1], %[mr1], v252\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr1], %[lr1], v255\n" \
  "v_mul_f32 v106, v106, v255\n" \
  "v_mul_f32 v107, v107, v255\n" \
  "v_mul_f32 v108, v108, v255\n" \
  "v_mul_f32 v109, v109, v255\n" \
  "v_mul_f32 v110, v110, v255\n" \
  "v_mul_f32 v111, v111, v255\n" \
  "v_mul_f32 v112, v112, v255\n" \
  "v_mul_f32 v113, v113, v255\n" \
  "v_mul_f32 v114, v114, v255\n" \
  "v_mul_f32 v115, v115, v255\n" \
  "v_mul_f32 v116, v116, v255\n" \
  "v_mul_f32 v117, v117, v255\n" \
  "v_mul_f32 v118, v118, v255\n" \
  "v_mul_f32 v119, v119, v255\n" \
  "v_mul_f32 v120, v120, v255\n" \
  "v_mul_f32 v121, v121, v255\n" \
  "v_mul_f32 v122, v122, v255\n" \
  "v_mul_f32 v123, v123, v255\n" \
  "v_mul_f32 v124, v124, v255\n" \
  "v_mul_f32 v125, v125, v255\n" \
  "v_mul_f32 v126, v126, v255\n" \
  "v_mul_f32 v127, v127, v255\n" \
  "v_mul_f32 v128, v128, v255\n" \
  "v_mul_f32 v129, v129, v255\n" \
  "v_mul_f32 v130, v130, v255\n" \
  "v_mul_f32 v131, v131, v255\n" \
  "v_mul_f32 v132, v132, v255\n" \
  "v_mul_f32 v133, v133, v255\n" \
  "v_mul_f32 v134, v134, v255\n" \
  "v_mul_f32 v135, v135, v255\n" \
  "v_mul_f32 v136, v136, v255\n" \
  "v_mul_f32 v137, v137, v255\n" \
  "v_sub_f32 v186, v186, v252\n" \
  "v_sub_f32 v187, v187, v252\n" \
  "v_sub_f32 v188, v188, v252\n" \
  "v_sub_f32 v189, v189, v252\n" \
  "v_sub_f32 v190, v190, v252\n" \
  "v_sub_f32 v191, v191, v252\n" \
  "v_sub_f32 v192, v192, v252\n" \
  "v_sub_f32 v193, v193, v252\n" \
  "v_sub_f32 v194, v194, v252\n" \
  "v_sub_f32 v195, v195, v252\n" \
  "v_sub_f32 v196, v196, v252\n" \
  "v_sub_f32 v197, v197, v252\n" \
  "v_sub_f32 v198, v198, v252\n" \
  "v_sub_f32 v199, v199, v252\n" \
  "v_sub_f32 v200, v200, v252\n" \
  "v_sub_f32 v201, v201, v252\n" \
  "v_sub_f32 v154, v154, v252\n" \
  "v_sub_f32 v155, v155, v252\n" \
  "v_sub_f32 v156, v156, v252\n" \
  "v_sub_f32 v157, v157, v252\n" \
  "v_sub_f32 v158, v158, v252\n" \
  "v_sub_f32 v159, v159, v252\n" \
  "v_sub_f32 v160, v160, v252\n" \
  "v_sub_f32 v161, v161, v252\n" \
  "v_sub_f32 v162, v162, v252\n" \
  "v_sub_f32 v163, v163, v252\n" \
  "v_sub_f32 v164, v164, v252\n" \
  "v_sub_f32 v165, v165, v252\n" \
  "v_sub_f32 v166, v166, v252\n" \
  "v_sub_f32 v167, v167, v252\n" \
  "v_sub_f32 v168, v168, v252\n" \
  "v_sub_f32 v169, v169, v252\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_add_f32 v254, v250, v251\n" \
  "v_exp_f32 v250, v156\n" \
  "v_exp_f32 v251, v157\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v211, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v160\n" \
  "v_exp_f32 v251, v161\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v213, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v164\n" \
  "v_exp_f32 v251, v165\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v215, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v168\n" \
  "v_exp_f32 v251, v169\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v217, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_mask0_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_sub_u32 v255, s38, %[hi4]\n" \
  "v_mov_b32 v69, 0xff800000\n" \
  "v_cmp_ge_i32 vcc, 0, v255\n" \
  "v_cndmask_b32 v138, v138, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 1, v255\n" \
  "v_cndmask_b32 v139, v139, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 2, v255\n" \
  "v_cndmask_b32 v140, v140, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 3, v255\n" \
  "v_cndmask_b32 v141, v141, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 8, v255\n" \
  "v_cndmask_b32 v142, v142, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 9, v255\n" \
  "v_cndmask_b32 v143, v143, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 10, v255\n" \
  "v_cndmask_b32 v144, v144, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 11, v255\n" \
  "v_cndmask_b32 v145, v145, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 16, v255\n" \
  "v_cndmask_b32 v146, v146, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 17, v255\n" \
  "v_cndmask_b32 v147, v147, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 18, v255\n" \
  "v_cndmask_b32 v148, v148, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 19, v255\n" \
  "v_cndmask_b32 v149, v149, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 24, v255\n" \
  "v_cndmask_b32 v150, v150, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 25, v255\n" \
  "v_cndmask_b32 v151, v151, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 26, v255\n" \
  "v_cndmask_b32 v152, v152, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 27, v255\n" \
  "v_cndmask_b32 v153, v153, v69, vcc\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_mask1_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_sub_u32 v255, s38, %[hi4]\n" \
  "v_mov_b32 v69, 0xff800000\n" \
  "v_cmp_ge_i32 vcc, 0, v255\n" \
  "v_cndmask_b32 v154, v154, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 1, v255\n" \
  "v_cndmask_b32 v155, v155, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 2, v255\n" \
  "v_cndmask_b32 v156, v156, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 3, v255\n" \
  "v_cndmask_b32 v157, v157, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 8, v255\n" \
  "v_cndmask_b32 v158, v158, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 9, v255\n" \
  "v_cndmask_b32 v159, v159, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 10, v255\n" \
  "v_cndmask_b32 v160, v160, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 11, v255\n" \
  "v_cndmask_b32 v161, v161, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 16, v255\n" \
  "v_cndmask_b32 v162, v162, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 17, v255\n" \
  "v_cndmask_b32 v163, v163, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 18, v255\n" \
  "v_cndmask_b32 v164, v164, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 19, v255\n" \
  "v_cndmask_b32 v165, v165, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 24, v255\n" \
  "v_cndmask_b32 v166, v166, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 25, v255\n" \
  "v_cndmask_b32 v167, v167, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 26, v255\n" \
  "v_cndmask_b32 v168, v168, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 27, v255\n" \
  "v_cndmask_b32 v169, v169, v69, vcc\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_end_%=:\n"
// clang-format on
#define FLASH_DP2_ASM_CLOBBERS \
  "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", \
  "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", \
  "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", \
  "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", \
  "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", \
  "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", \
  "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", \
  "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", \
  "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", \
  "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", \
  "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", \
  "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", \
  "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", \
  "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", \
  "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", \
  "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", \
  "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", \
  "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", \
  "v252", "v253", "v254", "v255", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", \
  "s44", "s45", "vcc", "scc", "memory"
// clang-format off
#define FLASH_DP2_ASM_TEXT_X \
  "v_add_u32 v70, %[lds], %[ab0]\n" \
  "v_xor_b32 v71, 32, v70\n" \
  "v_xor_b32 v72, 64, v70\n" \
  "v_xor_b32 v73, 96, v70\n" \
  "global_load_dwordx4 v[36:39], %[qa0], off offset:0\n" \
  "global_load_dwordx4 v[40:43], %[qa0], off offset:32\n" \
  "global_load_dwordx4 v[44:47], %[qa0], off offset:64\n" \
  "global_load_dwordx4 v[48:51], %[qa0], off offset:96\n" \
  "global_load_dwordx4 v[52:55], %[qa1], off offset:0\n" \
  "global_load_dwordx4 v[56:59], %[qa1], off offset:32\n" \
  "global_load_dwordx4 v[60:63], %[qa1], off offset:64\n" \
  "global_load_dwordx4 v[64:67], %[qa1], off offset:96\n" \
  "global_load_dwordx2 v[186:187], %[vxa], off offset:0\n" \
  "global_load_dwordx2 v[188:189], %[vxa], off offset:16\n" \
  "global_load_dwordx2 v[190:191], %[vxa], off offset:32\n" \
  "global_load_dwordx2 v[192:193], %[vxa], off offset:48\n" \
  "global_load_dwordx2 v[194:195], %[vxa], off offset:64\n" \
  "global_load_dwordx2 v[196:197], %[vxa], off offset:80\n" \
  "global_load_dwordx2 v[198:199], %[vxa], off offset:96\n" \
  "global_load_dwordx2 v[200:201], %[vxa], off offset:112\n" \
  "global_load_dwordx4 v[154:157], %[kxa], off offset:0\n" \
  "global_load_dwordx4 v[158:161], %[kxa], off offset:32\n" \
  "global_load_dwordx4 v[162:165], %[kxa], off offset:64\n" \
  "global_load_dwordx4 v[166:169], %[kxa], off offset:96\n" \
  "s_mov_b32 s36, 0\n" \
  "s_mov_b32 s37, 0\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 m0, %[dma_base], 0\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 1024\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 8192\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 9216\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "s_add_u32 s37, s37, 1\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 m0, %[dma_base], 16384\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 17408\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 24576\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 25600\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "s_add_u32 s37, s37, 1\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 m0, %[dma_base], 32768\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 33792\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 40960\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "s_add_u32 m0, %[dma_base], 41984\n" \
  "s_nop 0\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "s_add_u32 s37, s37, 1\n" \
  "v_mov_b32 v210, 0xff800000\n" \
  "v_mov_b32 v211, 0xff800000\n" \
  "s_cmp_eq_u32 %[xflag], 0\n" \
  "s_cbranch_scc1 .Lfd2_nox_%=\n" \
  "s_waitcnt vmcnt(12)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[154:157], v[36:39], 0\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[158:161], v[40:43], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[162:165], v[44:47], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[166:169], v[48:51], v[138:153]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_mov_b32 v210, v138\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[154:157], v[52:55], 0\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[158:161], v[56:59], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[162:165], v[60:63], v[138:153]\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[166:169], v[64:67], v[138:153]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_mov_b32 v211, v138\n" \
  ".Lfd2_nox_%=:\n" \
  "s_waitcnt vmcnt(8)\n" \
  "s_barrier\n" \
  "s_mov_b32 s38, %[seq]\n" \
  "ds_read_b128 v[218:221], v70 offset:0\n" \
  "ds_read_b128 v[222:225], v71 offset:0\n" \
  "ds_read_b128 v[226:229], v72 offset:0\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], 0\n" \
  "ds_read_b128 v[230:233], v73 offset:0\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[222:225], v[40:43], v[138:153]\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[44:47], v[138:153]\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[230:233], v[48:51], v[138:153]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask1_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc2_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret2_%=-.Lfd2_pc2_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret2_%=:\n" \
  ".Lfd2_nomask1_%=:\n" \
  "v_max3_f32 v252, v138, v139, v140\n" \
  "v_max3_f32 v253, v141, v142, v143\n" \
  "v_max3_f32 v255, v144, v145, v146\n" \
  "v_max3_f32 v69, v147, v148, v149\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v150, v151, v152\n" \
  "v_max3_f32 v69, v69, v253, v153\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, v252, v210\n" \
  "v_mul_f32 %[mr0], %[scale], v252\n" \
  "v_sub_f32 v255, v210, v252\n" \
  "v_mul_f32 v255, %[scale], v255\n" \
  "v_exp_f32 v255, v255\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr0], 0.5, v255\n" \
  "v_lshlrev_b32 v253, 16, v186\n" \
  "v_mul_f32 v74, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v186\n" \
  "v_mul_f32 v75, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v187\n" \
  "v_mul_f32 v76, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v187\n" \
  "v_mul_f32 v77, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v188\n" \
  "v_mul_f32 v78, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v188\n" \
  "v_mul_f32 v79, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v189\n" \
  "v_mul_f32 v80, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v189\n" \
  "v_mul_f32 v81, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v190\n" \
  "v_mul_f32 v82, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v190\n" \
  "v_mul_f32 v83, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v191\n" \
  "v_mul_f32 v84, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v191\n" \
  "v_mul_f32 v85, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v192\n" \
  "v_mul_f32 v86, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v192\n" \
  "v_mul_f32 v87, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v193\n" \
  "v_mul_f32 v88, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v193\n" \
  "v_mul_f32 v89, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v194\n" \
  "v_mul_f32 v90, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v194\n" \
  "v_mul_f32 v91, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v195\n" \
  "v_mul_f32 v92, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v195\n" \
  "v_mul_f32 v93, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v196\n" \
  "v_mul_f32 v94, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v196\n" \
  "v_mul_f32 v95, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v197\n" \
  "v_mul_f32 v96, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v197\n" \
  "v_mul_f32 v97, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v198\n" \
  "v_mul_f32 v98, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v198\n" \
  "v_mul_f32 v99, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v199\n" \
  "v_mul_f32 v100, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v199\n" \
  "v_mul_f32 v101, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v200\n" \
  "v_mul_f32 v102, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v200\n" \
  "v_mul_f32 v103, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v201\n" \
  "v_mul_f32 v104, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v201\n" \
  "v_mul_f32 v105, v255, v253\n" \
  "v_sub_f32 v170, 0, v252\n" \
  "v_sub_f32 v171, 0, v252\n" \
  "v_sub_f32 v172, 0, v252\n" \
  "v_sub_f32 v173, 0, v252\n" \
  "v_sub_f32 v174, 0, v252\n" \
  "v_sub_f32 v175, 0, v252\n" \
  "v_sub_f32 v176, 0, v252\n" \
  "v_sub_f32 v177, 0, v252\n" \
  "v_sub_f32 v178, 0, v252\n" \
  "v_sub_f32 v179, 0, v252\n" \
  "v_sub_f32 v180, 0, v252\n" \
  "v_sub_f32 v181, 0, v252\n" \
  "v_sub_f32 v182, 0, v252\n" \
  "v_sub_f32 v183, 0, v252\n" \
  "v_sub_f32 v184, 0, v252\n" \
  "v_sub_f32 v185, 0, v252\n" \
  "v_sub_f32 v138, v138, v252\n" \
  "v_sub_f32 v139, v139, v252\n" \
  "v_sub_f32 v140, v140, v252\n" \
  "v_sub_f32 v141, v141, v252\n" \
  "v_sub_f32 v142, v142, v252\n" \
  "v_sub_f32 v143, v143, v252\n" \
  "v_sub_f32 v144, v144, v252\n" \
  "v_sub_f32 v145, v145, v252\n" \
  "v_sub_f32 v146, v146, v252\n" \
  "v_sub_f32 v147, v147, v252\n" \
  "v_sub_f32 v148, v148, v252\n" \
  "v_sub_f32 v149, v149, v252\n" \
  "v_sub_f32 v150, v150, v252\n" \
  "v_sub_f32 v151, v151, v252\n" \
  "v_sub_f32 v152, v152, v252\n" \
  "v_sub_f32 v153, v153, v252\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], 0\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[222:225], v[56:59], v[154:169]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[230:233], v[64:67], v[154:169]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:4096\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:8192\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:4096\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok3_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc4_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret4_%=-.Lfd2_pc4_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret4_%=:\n" \
  ".Lfd2_ok3_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask5_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc6_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret6_%=-.Lfd2_pc6_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret6_%=:\n" \
  ".Lfd2_nomask5_%=:\n" \
  "v_max3_f32 v252, v154, v155, v156\n" \
  "v_max3_f32 v253, v157, v158, v159\n" \
  "v_max3_f32 v255, v160, v161, v162\n" \
  "v_max3_f32 v69, v163, v164, v165\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v166, v167, v168\n" \
  "v_max3_f32 v69, v69, v253, v169\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, v252, v211\n" \
  "v_mul_f32 %[mr1], %[scale], v252\n" \
  "v_sub_f32 v255, v211, v252\n" \
  "v_mul_f32 v255, %[scale], v255\n" \
  "v_exp_f32 v255, v255\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr1], 0.5, v255\n" \
  "v_lshlrev_b32 v253, 16, v186\n" \
  "v_mul_f32 v106, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v186\n" \
  "v_mul_f32 v107, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v187\n" \
  "v_mul_f32 v108, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v187\n" \
  "v_mul_f32 v109, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v188\n" \
  "v_mul_f32 v110, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v188\n" \
  "v_mul_f32 v111, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v189\n" \
  "v_mul_f32 v112, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v189\n" \
  "v_mul_f32 v113, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v190\n" \
  "v_mul_f32 v114, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v190\n" \
  "v_mul_f32 v115, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v191\n" \
  "v_mul_f32 v116, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v191\n" \
  "v_mul_f32 v117, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v192\n" \
  "v_mul_f32 v118, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v192\n" \
  "v_mul_f32 v119, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v193\n" \
  "v_mul_f32 v120, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v193\n" \
  "v_mul_f32 v121, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v194\n" \
  "v_mul_f32 v122, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v194\n" \
  "v_mul_f32 v123, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v195\n" \
  "v_mul_f32 v124, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v195\n" \
  "v_mul_f32 v125, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v196\n" \
  "v_mul_f32 v126, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v196\n" \
  "v_mul_f32 v127, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v197\n" \
  "v_mul_f32 v128, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v197\n" \
  "v_mul_f32 v129, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v198\n" \
  "v_mul_f32 v130, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v198\n" \
  "v_mul_f32 v131, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v199\n" \
  "v_mul_f32 v132, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v199\n" \
  "v_mul_f32 v133, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v200\n" \
  "v_mul_f32 v134, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v200\n" \
  "v_mul_f32 v135, v255, v253\n" \
  "v_lshlrev_b32 v253, 16, v201\n" \
  "v_mul_f32 v136, v255, v253\n" \
  "v_and_b32 v253, 0xffff0000, v201\n" \
  "v_mul_f32 v137, v255, v253\n" \
  "v_sub_f32 v186, 0, v252\n" \
  "v_sub_f32 v187, 0, v252\n" \
  "v_sub_f32 v188, 0, v252\n" \
  "v_sub_f32 v189, 0, v252\n" \
  "v_sub_f32 v190, 0, v252\n" \
  "v_sub_f32 v191, 0, v252\n" \
  "v_sub_f32 v192, 0, v252\n" \
  "v_sub_f32 v193, 0, v252\n" \
  "v_sub_f32 v194, 0, v252\n" \
  "v_sub_f32 v195, 0, v252\n" \
  "v_sub_f32 v196, 0, v252\n" \
  "v_sub_f32 v197, 0, v252\n" \
  "v_sub_f32 v198, 0, v252\n" \
  "v_sub_f32 v199, 0, v252\n" \
  "v_sub_f32 v200, 0, v252\n" \
  "v_sub_f32 v201, 0, v252\n" \
  "v_sub_f32 v154, v154, v252\n" \
  "v_sub_f32 v155, v155, v252\n" \
  "v_sub_f32 v156, v156, v252\n" \
  "v_sub_f32 v157, v157, v252\n" \
  "v_sub_f32 v158, v158, v252\n" \
  "v_sub_f32 v159, v159, v252\n" \
  "v_sub_f32 v160, v160, v252\n" \
  "v_sub_f32 v161, v161, v252\n" \
  "v_sub_f32 v162, v162, v252\n" \
  "v_sub_f32 v163, v163, v252\n" \
  "v_sub_f32 v164, v164, v252\n" \
  "v_sub_f32 v165, v165, v252\n" \
  "v_sub_f32 v166, v166, v252\n" \
  "v_sub_f32 v167, v167, v252\n" \
  "v_sub_f32 v168, v168, v252\n" \
  "v_sub_f32 v169, v169, v252\n" \
  ".p2align 6\n" \
  ".Lfd2_loop_%=:\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:12288\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:4096\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:8192\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:4096\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:12288\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok7_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc8_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret8_%=-.Lfd2_pc8_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret8_%=:\n" \
  ".Lfd2_ok7_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask9_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc10_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret10_%=-.Lfd2_pc10_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret10_%=:\n" \
  ".Lfd2_nomask9_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok11_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc12_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret12_%=-.Lfd2_pc12_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret12_%=:\n" \
  ".Lfd2_ok11_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask13_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc14_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret14_%=-.Lfd2_pc14_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret14_%=:\n" \
  ".Lfd2_nomask13_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 8192\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:16384\n" \
  "ds_read_b128 v[222:225], v72 offset:8192\n" \
  "ds_read_b128 v[226:229], v71 offset:16384\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:12288\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "s_add_u32 m0, %[dma_base], 49152\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:16384\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:8192\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 50176\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:16384\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:12288\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 57344\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 58368\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok15_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc16_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret16_%=-.Lfd2_pc16_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret16_%=:\n" \
  ".Lfd2_ok15_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask17_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc18_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret18_%=-.Lfd2_pc18_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret18_%=:\n" \
  ".Lfd2_nomask17_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:20480\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:24576\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:20480\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok19_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc20_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret20_%=-.Lfd2_pc20_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret20_%=:\n" \
  ".Lfd2_ok19_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask21_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc22_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret22_%=-.Lfd2_pc22_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret22_%=:\n" \
  ".Lfd2_nomask21_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:28672\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:20480\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:24576\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:20480\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:28672\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok23_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc24_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret24_%=-.Lfd2_pc24_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret24_%=:\n" \
  ".Lfd2_ok23_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask25_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc26_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret26_%=-.Lfd2_pc26_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret26_%=:\n" \
  ".Lfd2_nomask25_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok27_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc28_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret28_%=-.Lfd2_pc28_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret28_%=:\n" \
  ".Lfd2_ok27_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask29_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc30_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret30_%=-.Lfd2_pc30_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret30_%=:\n" \
  ".Lfd2_nomask29_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 24576\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:32768\n" \
  "ds_read_b128 v[222:225], v72 offset:24576\n" \
  "ds_read_b128 v[226:229], v71 offset:32768\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:28672\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "s_add_u32 m0, %[dma_base], 0\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:32768\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:24576\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 1024\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:32768\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:28672\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 8192\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 9216\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok31_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc32_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret32_%=-.Lfd2_pc32_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret32_%=:\n" \
  ".Lfd2_ok31_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask33_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc34_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret34_%=-.Lfd2_pc34_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret34_%=:\n" \
  ".Lfd2_nomask33_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:36864\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:40960\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:36864\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok35_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc36_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret36_%=-.Lfd2_pc36_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret36_%=:\n" \
  ".Lfd2_ok35_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask37_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc38_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret38_%=-.Lfd2_pc38_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret38_%=:\n" \
  ".Lfd2_nomask37_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:45056\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:36864\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:40960\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:36864\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:45056\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok39_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc40_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret40_%=-.Lfd2_pc40_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret40_%=:\n" \
  ".Lfd2_ok39_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask41_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc42_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret42_%=-.Lfd2_pc42_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret42_%=:\n" \
  ".Lfd2_nomask41_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok43_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc44_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret44_%=-.Lfd2_pc44_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret44_%=:\n" \
  ".Lfd2_ok43_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask45_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc46_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret46_%=-.Lfd2_pc46_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret46_%=:\n" \
  ".Lfd2_nomask45_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 40960\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:49152\n" \
  "ds_read_b128 v[222:225], v72 offset:40960\n" \
  "ds_read_b128 v[226:229], v71 offset:49152\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:45056\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "s_add_u32 m0, %[dma_base], 16384\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:49152\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:40960\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 17408\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:49152\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:45056\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 24576\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 25600\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok47_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc48_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret48_%=-.Lfd2_pc48_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret48_%=:\n" \
  ".Lfd2_ok47_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask49_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc50_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret50_%=-.Lfd2_pc50_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret50_%=:\n" \
  ".Lfd2_nomask49_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:53248\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:57344\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:53248\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok51_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc52_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret52_%=-.Lfd2_pc52_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret52_%=:\n" \
  ".Lfd2_ok51_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask53_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc54_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret54_%=-.Lfd2_pc54_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret54_%=:\n" \
  ".Lfd2_nomask53_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_lshl_b32 s39, s36, 6\n" \
  "s_sub_i32 s38, %[seq], s39\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v70 offset:61440\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:53248\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v71 offset:57344\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:53248\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v71 offset:61440\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok55_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc56_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret56_%=-.Lfd2_pc56_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret56_%=:\n" \
  ".Lfd2_ok55_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask57_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc58_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret58_%=-.Lfd2_pc58_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret58_%=:\n" \
  ".Lfd2_nomask57_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok59_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc60_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret60_%=-.Lfd2_pc60_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret60_%=:\n" \
  ".Lfd2_ok59_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask61_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc62_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret62_%=-.Lfd2_pc62_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret62_%=:\n" \
  ".Lfd2_nomask61_%=:\n" \
  "s_add_u32 s39, s36, 1\n" \
  "s_cmp_eq_u32 s39, %[ntile]\n" \
  "s_mov_b32 s43, 57344\n" \
  "s_cbranch_scc1 .Lfd2_epi_%=\n" \
  "s_waitcnt vmcnt(4)\n" \
  "s_barrier\n" \
  "s_sub_i32 s38, s38, 32\n" \
  "s_mul_i32 s41, s37, %[ktile]\n" \
  "s_lshl_b32 s42, s37, 7\n" \
  "s_cmp_ge_u32 s37, %[ntile]\n" \
  "s_cselect_b32 s41, 0x7ff00000, s41\n" \
  "s_cselect_b32 s42, 0x7ff00000, s42\n" \
  "s_add_u32 s37, s37, 1\n" \
  "ds_read_b128 v[218:221], v70 offset:0\n" \
  "ds_read_b128 v[222:225], v72 offset:57344\n" \
  "ds_read_b128 v[226:229], v71 offset:0\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[218:221], v[36:39], v[170:185]\n" \
  "ds_read_b128 v[230:233], v72 offset:61440\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "s_add_u32 m0, %[dma_base], 32768\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[222:225], v[202:205], v[74:89]\n" \
  "ds_read_b128 v[234:237], v72 offset:0\n" \
  "buffer_load_dwordx4 %[ko0], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[226:229], v[40:43], v[138:153]\n" \
  "ds_read_b128 v[238:241], v73 offset:57344\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 33792\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[202:205], v[90:105]\n" \
  "ds_read_b128 v[242:245], v73 offset:0\n" \
  "buffer_load_dwordx4 %[ko1], %[rsk], s41 offen lds\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[234:237], v[44:47], v[138:153]\n" \
  "ds_read_b128 v[246:249], v73 offset:61440\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 40960\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[238:241], v[206:209], v[74:89]\n" \
  "buffer_load_dwordx4 %[vo0], %[rsv], s42 offen lds\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[138:153], v[242:245], v[48:51], v[138:153]\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "s_add_u32 m0, %[dma_base], 41984\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[246:249], v[206:209], v[90:105]\n" \
  "buffer_load_dwordx4 %[vo1], %[rsv], s42 offen lds\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok63_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc64_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret64_%=-.Lfd2_pc64_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret64_%=:\n" \
  ".Lfd2_ok63_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask65_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc66_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret66_%=-.Lfd2_pc66_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask0_%=\n" \
  ".Lfd2_ret66_%=:\n" \
  ".Lfd2_nomask65_%=:\n" \
  "v_mul_f32 v138, %[scale], v138\n" \
  "v_mul_f32 v139, %[scale], v139\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[218:221], v[52:55], v[186:201]\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "v_mul_f32 v140, %[scale], v140\n" \
  "v_mul_f32 v141, %[scale], v141\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[222:225], v[210:213], v[106:121]\n" \
  "v_exp_f32 v252, v140\n" \
  "v_exp_f32 v253, v141\n" \
  "v_mul_f32 v142, %[scale], v142\n" \
  "v_mul_f32 v143, %[scale], v143\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[226:229], v[56:59], v[154:169]\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "v_mul_f32 v144, %[scale], v144\n" \
  "v_mul_f32 v145, %[scale], v145\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v203, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[210:213], v[122:137]\n" \
  "v_exp_f32 v252, v144\n" \
  "v_exp_f32 v253, v145\n" \
  "v_mul_f32 v146, %[scale], v146\n" \
  "v_mul_f32 v147, %[scale], v147\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[234:237], v[60:63], v[154:169]\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "v_mul_f32 v148, %[scale], v148\n" \
  "v_mul_f32 v149, %[scale], v149\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v205, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[238:241], v[214:217], v[106:121]\n" \
  "v_exp_f32 v252, v148\n" \
  "v_exp_f32 v253, v149\n" \
  "ds_read_b128 v[218:221], v70 offset:4096\n" \
  "v_mul_f32 v150, %[scale], v150\n" \
  "v_mul_f32 v151, %[scale], v151\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_mfma_f32_32x32x16_bf16 v[154:169], v[242:245], v[64:67], v[154:169]\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "ds_read_b128 v[222:225], v70 offset:8192\n" \
  "v_mul_f32 v152, %[scale], v152\n" \
  "v_mul_f32 v153, %[scale], v153\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v207, v252, v253\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[246:249], v[214:217], v[122:137]\n" \
  "v_exp_f32 v252, v152\n" \
  "v_exp_f32 v253, v153\n" \
  "ds_read_b128 v[226:229], v71 offset:4096\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v209, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok67_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc68_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret68_%=-.Lfd2_pc68_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow0_%=\n" \
  ".Lfd2_ret68_%=:\n" \
  ".Lfd2_ok67_%=:\n" \
  "v_add_f32 %[lr0], %[lr0], v254\n" \
  "s_cmp_ge_i32 s38, 32\n" \
  "s_cbranch_scc1 .Lfd2_nomask69_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc70_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret70_%=-.Lfd2_pc70_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_mask1_%=\n" \
  ".Lfd2_ret70_%=:\n" \
  ".Lfd2_nomask69_%=:\n" \
  "s_add_u32 s36, s36, 1\n" \
  "s_branch .Lfd2_loop_%=\n" \
  ".Lfd2_epi_%=:\n" \
  "v_add_u32 v69, s43, v72\n" \
  "ds_read_b128 v[218:221], v69 offset:0\n" \
  "v_add_u32 v69, s43, v72\n" \
  "ds_read_b128 v[222:225], v69 offset:4096\n" \
  "v_add_u32 v69, s43, v73\n" \
  "ds_read_b128 v[226:229], v69 offset:0\n" \
  "v_mul_f32 v154, %[scale], v154\n" \
  "v_mul_f32 v155, %[scale], v155\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[218:221], v[202:205], v[74:89]\n" \
  "v_add_u32 v69, s43, v73\n" \
  "ds_read_b128 v[230:233], v69 offset:4096\n" \
  "v_mul_f32 v156, %[scale], v156\n" \
  "v_mul_f32 v157, %[scale], v157\n" \
  "v_exp_f32 v252, v156\n" \
  "v_exp_f32 v253, v157\n" \
  "s_waitcnt lgkmcnt(2)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[222:225], v[202:205], v[90:105]\n" \
  "v_mul_f32 v158, %[scale], v158\n" \
  "v_mul_f32 v159, %[scale], v159\n" \
  "v_mov_b32 v254, v250\n" \
  "v_mov_b32 v255, v251\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_waitcnt lgkmcnt(1)\n" \
  "v_mfma_f32_32x32x16_bf16 v[74:89], v[226:229], v[206:209], v[74:89]\n" \
  "v_mul_f32 v160, %[scale], v160\n" \
  "v_mul_f32 v161, %[scale], v161\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v211, v252, v253\n" \
  "v_exp_f32 v252, v160\n" \
  "v_exp_f32 v253, v161\n" \
  "s_waitcnt lgkmcnt(0)\n" \
  "v_mfma_f32_32x32x16_bf16 v[90:105], v[230:233], v[206:209], v[90:105]\n" \
  "v_mul_f32 v162, %[scale], v162\n" \
  "v_mul_f32 v163, %[scale], v163\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "v_mul_f32 v164, %[scale], v164\n" \
  "v_mul_f32 v165, %[scale], v165\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v213, v252, v253\n" \
  "v_exp_f32 v252, v164\n" \
  "v_exp_f32 v253, v165\n" \
  "v_mul_f32 v166, %[scale], v166\n" \
  "v_mul_f32 v167, %[scale], v167\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "v_mul_f32 v168, %[scale], v168\n" \
  "v_mul_f32 v169, %[scale], v169\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v215, v252, v253\n" \
  "v_exp_f32 v252, v168\n" \
  "v_exp_f32 v253, v169\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v255, v255, v251\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v252\n" \
  "v_add_f32 v255, v255, v253\n" \
  "v_cvt_pk_bf16_f32 v217, v252, v253\n" \
  "v_add_f32 v254, v254, v255\n" \
  "v_cmp_lt_f32 vcc, 0x5f800000, v254\n" \
  "s_cbranch_vccz .Lfd2_ok71_%=\n" \
  "s_getpc_b64 s[44:45]\n" \
  ".Lfd2_pc72_%=:\n" \
  "s_add_u32 s44, s44, .Lfd2_ret72_%=-.Lfd2_pc72_%=\n" \
  "s_addc_u32 s45, s45, 0\n" \
  "s_branch .Lfd2_slow1_%=\n" \
  ".Lfd2_ret72_%=:\n" \
  ".Lfd2_ok71_%=:\n" \
  "v_add_f32 %[lr1], %[lr1], v254\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[218:221], v[210:213], v[106:121]\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[222:225], v[210:213], v[122:137]\n" \
  "v_mfma_f32_32x32x16_bf16 v[106:121], v[226:229], v[214:217], v[106:121]\n" \
  "v_mfma_f32_32x32x16_bf16 v[122:137], v[230:233], v[214:217], v[122:137]\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n" \
  "s_barrier\n" \
  "ds_write_b128 %[dump], v[74:77] offset:0\n" \
  "ds_write_b128 %[dump], v[78:81] offset:1024\n" \
  "ds_write_b128 %[dump], v[82:85] offset:2048\n" \
  "ds_write_b128 %[dump], v[86:89] offset:3072\n" \
  "ds_write_b128 %[dump], v[90:93] offset:4096\n" \
  "ds_write_b128 %[dump], v[94:97] offset:5120\n" \
  "ds_write_b128 %[dump], v[98:101] offset:6144\n" \
  "ds_write_b128 %[dump], v[102:105] offset:7168\n" \
  "ds_write_b128 %[dump], v[106:109] offset:8192\n" \
  "ds_write_b128 %[dump], v[110:113] offset:9216\n" \
  "ds_write_b128 %[dump], v[114:117] offset:10240\n" \
  "ds_write_b128 %[dump], v[118:121] offset:11264\n" \
  "ds_write_b128 %[dump], v[122:125] offset:12288\n" \
  "ds_write_b128 %[dump], v[126:129] offset:13312\n" \
  "ds_write_b128 %[dump], v[130:133] offset:14336\n" \
  "ds_write_b128 %[dump], v[134:137] offset:15360\n" \
  "s_waitcnt vmcnt(0) lgkmcnt(0)\n" \
  "v_mbcnt_lo_u32_b32 %[lid], -1, 0\n" \
  "v_mbcnt_hi_u32_b32 %[lid], -1, %[lid]\n" \
  "s_branch .Lfd2_end_%=\n" \
  ".Lfd2_slow0_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_max3_f32 v252, v138, v139, v140\n" \
  "v_max3_f32 v253, v141, v142, v143\n" \
  "v_max3_f32 v255, v144, v145, v146\n" \
  "v_max3_f32 v69, v147, v148, v149\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v150, v151, v152\n" \
  "v_max3_f32 v69, v69, v253, v153\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, 0, v252\n" \
  "v_sub_f32 v255, 0, v252\n" \
  "v_exp_f32 v255, v255\n" \
  "v_add_f32 %[mr0], %[mr0], v252\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr0], %[lr0], v255\n" \
  "v_mul_f32 v74, v74, v255\n" \
  "v_mul_f32 v75, v75, v255\n" \
  "v_mul_f32 v76, v76, v255\n" \
  "v_mul_f32 v77, v77, v255\n" \
  "v_mul_f32 v78, v78, v255\n" \
  "v_mul_f32 v79, v79, v255\n" \
  "v_mul_f32 v80, v80, v255\n" \
  "v_mul_f32 v81, v81, v255\n" \
  "v_mul_f32 v82, v82, v255\n" \
  "v_mul_f32 v83, v83, v255\n" \
  "v_mul_f32 v84, v84, v255\n" \
  "v_mul_f32 v85, v85, v255\n" \
  "v_mul_f32 v86, v86, v255\n" \
  "v_mul_f32 v87, v87, v255\n" \
  "v_mul_f32 v88, v88, v255\n" \
  "v_mul_f32 v89, v89, v255\n" \
  "v_mul_f32 v90, v90, v255\n" \
  "v_mul_f32 v91, v91, v255\n" \
  "v_mul_f32 v92, v92, v255\n" \
  "v_mul_f32 v93, v93, v255\n" \
  "v_mul_f32 v94, v94, v255\n" \
  "v_mul_f32 v95, v95, v255\n" \
  "v_mul_f32 v96, v96, v255\n" \
  "v_mul_f32 v97, v97, v255\n" \
  "v_mul_f32 v98, v98, v255\n" \
  "v_mul_f32 v99, v99, v255\n" \
  "v_mul_f32 v100, v100, v255\n" \
  "v_mul_f32 v101, v101, v255\n" \
  "v_mul_f32 v102, v102, v255\n" \
  "v_mul_f32 v103, v103, v255\n" \
  "v_mul_f32 v104, v104, v255\n" \
  "v_mul_f32 v105, v105, v255\n" \
  "v_mul_f32 v69, %[rscale], v252\n" \
  "v_sub_f32 v170, v170, v69\n" \
  "v_sub_f32 v171, v171, v69\n" \
  "v_sub_f32 v172, v172, v69\n" \
  "v_sub_f32 v173, v173, v69\n" \
  "v_sub_f32 v174, v174, v69\n" \
  "v_sub_f32 v175, v175, v69\n" \
  "v_sub_f32 v176, v176, v69\n" \
  "v_sub_f32 v177, v177, v69\n" \
  "v_sub_f32 v178, v178, v69\n" \
  "v_sub_f32 v179, v179, v69\n" \
  "v_sub_f32 v180, v180, v69\n" \
  "v_sub_f32 v181, v181, v69\n" \
  "v_sub_f32 v182, v182, v69\n" \
  "v_sub_f32 v183, v183, v69\n" \
  "v_sub_f32 v184, v184, v69\n" \
  "v_sub_f32 v185, v185, v69\n" \
  "v_sub_f32 v138, v138, v252\n" \
  "v_sub_f32 v139, v139, v252\n" \
  "v_sub_f32 v140, v140, v252\n" \
  "v_sub_f32 v141, v141, v252\n" \
  "v_sub_f32 v142, v142, v252\n" \
  "v_sub_f32 v143, v143, v252\n" \
  "v_sub_f32 v144, v144, v252\n" \
  "v_sub_f32 v145, v145, v252\n" \
  "v_sub_f32 v146, v146, v252\n" \
  "v_sub_f32 v147, v147, v252\n" \
  "v_sub_f32 v148, v148, v252\n" \
  "v_sub_f32 v149, v149, v252\n" \
  "v_sub_f32 v150, v150, v252\n" \
  "v_sub_f32 v151, v151, v252\n" \
  "v_sub_f32 v152, v152, v252\n" \
  "v_sub_f32 v153, v153, v252\n" \
  "v_exp_f32 v250, v138\n" \
  "v_exp_f32 v251, v139\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v202, v250, v251\n" \
  "v_add_f32 v254, v250, v251\n" \
  "v_exp_f32 v250, v140\n" \
  "v_exp_f32 v251, v141\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v203, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v142\n" \
  "v_exp_f32 v251, v143\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v204, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v144\n" \
  "v_exp_f32 v251, v145\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v205, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v146\n" \
  "v_exp_f32 v251, v147\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v206, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v148\n" \
  "v_exp_f32 v251, v149\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v207, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v150\n" \
  "v_exp_f32 v251, v151\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v208, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v152\n" \
  "v_exp_f32 v251, v153\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v209, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_slow1_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_max3_f32 v252, v154, v155, v156\n" \
  "v_max3_f32 v253, v157, v158, v159\n" \
  "v_max3_f32 v255, v160, v161, v162\n" \
  "v_max3_f32 v69, v163, v164, v165\n" \
  "v_max3_f32 v252, v252, v253, v255\n" \
  "v_max3_f32 v253, v166, v167, v168\n" \
  "v_max3_f32 v69, v69, v253, v169\n" \
  "v_max_f32 v252, v252, v69\n" \
  "v_mov_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_permlane32_swap_b32 v253, v252\n" \
  "s_nop 1\n" \
  "v_max_f32 v252, v252, v253\n" \
  "v_max_f32 v252, 0, v252\n" \
  "v_sub_f32 v255, 0, v252\n" \
  "v_exp_f32 v255, v255\n" \
  "v_add_f32 %[mr1], %[mr1], v252\n" \
  "s_nop 0\n" \
  "v_mul_f32 %[lr1], %[lr1], v255\n" \
  "v_mul_f32 v106, v106, v255\n" \
  "v_mul_f32 v107, v107, v255\n" \
  "v_mul_f32 v108, v108, v255\n" \
  "v_mul_f32 v109, v109, v255\n" \
  "v_mul_f32 v110, v110, v255\n" \
  "v_mul_f32 v111, v111, v255\n" \
  "v_mul_f32 v112, v112, v255\n" \
  "v_mul_f32 v113, v113, v255\n" \
  "v_mul_f32 v114, v114, v255\n" \
  "v_mul_f32 v115, v115, v255\n" \
  "v_mul_f32 v116, v116, v255\n" \
  "v_mul_f32 v117, v117, v255\n" \
  "v_mul_f32 v118, v118, v255\n" \
  "v_mul_f32 v119, v119, v255\n" \
  "v_mul_f32 v120, v120, v255\n" \
  "v_mul_f32 v121, v121, v255\n" \
  "v_mul_f32 v122, v122, v255\n" \
  "v_mul_f32 v123, v123, v255\n" \
  "v_mul_f32 v124, v124, v255\n" \
  "v_mul_f32 v125, v125, v255\n" \
  "v_mul_f32 v126, v126, v255\n" \
  "v_mul_f32 v127, v127, v255\n" \
  "v_mul_f32 v128, v128, v255\n" \
  "v_mul_f32 v129, v129, v255\n" \
  "v_mul_f32 v130, v130, v255\n" \
  "v_mul_f32 v131, v131, v255\n" \
  "v_mul_f32 v132, v132, v255\n" \
  "v_mul_f32 v133, v133, v255\n" \
  "v_mul_f32 v134, v134, v255\n" \
  "v_mul_f32 v135, v135, v255\n" \
  "v_mul_f32 v136, v136, v255\n" \
  "v_mul_f32 v137, v137, v255\n" \
  "v_mul_f32 v69, %[rscale], v252\n" \
  "v_sub_f32 v186, v186, v69\n" \
  "v_sub_f32 v187, v187, v69\n" \
  "v_sub_f32 v188, v188, v69\n" \
  "v_sub_f32 v189, v189, v69\n" \
  "v_sub_f32 v190, v190, v69\n" \
  "v_sub_f32 v191, v191, v69\n" \
  "v_sub_f32 v192, v192, v69\n" \
  "v_sub_f32 v193, v193, v69\n" \
  "v_sub_f32 v194, v194, v69\n" \
  "v_sub_f32 v195, v195, v69\n" \
  "v_sub_f32 v196, v196, v69\n" \
  "v_sub_f32 v197, v197, v69\n" \
  "v_sub_f32 v198, v198, v69\n" \
  "v_sub_f32 v199, v199, v69\n" \
  "v_sub_f32 v200, v200, v69\n" \
  "v_sub_f32 v201, v201, v69\n" \
  "v_sub_f32 v154, v154, v252\n" \
  "v_sub_f32 v155, v155, v252\n" \
  "v_sub_f32 v156, v156, v252\n" \
  "v_sub_f32 v157, v157, v252\n" \
  "v_sub_f32 v158, v158, v252\n" \
  "v_sub_f32 v159, v159, v252\n" \
  "v_sub_f32 v160, v160, v252\n" \
  "v_sub_f32 v161, v161, v252\n" \
  "v_sub_f32 v162, v162, v252\n" \
  "v_sub_f32 v163, v163, v252\n" \
  "v_sub_f32 v164, v164, v252\n" \
  "v_sub_f32 v165, v165, v252\n" \
  "v_sub_f32 v166, v166, v252\n" \
  "v_sub_f32 v167, v167, v252\n" \
  "v_sub_f32 v168, v168, v252\n" \
  "v_sub_f32 v169, v169, v252\n" \
  "v_exp_f32 v250, v154\n" \
  "v_exp_f32 v251, v155\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v210, v250, v251\n" \
  "v_add_f32 v254, v250, v251\n" \
  "v_exp_f32 v250, v156\n" \
  "v_exp_f32 v251, v157\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v211, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v158\n" \
  "v_exp_f32 v251, v159\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v212, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v160\n" \
  "v_exp_f32 v251, v161\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v213, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v162\n" \
  "v_exp_f32 v251, v163\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v214, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v164\n" \
  "v_exp_f32 v251, v165\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v215, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v166\n" \
  "v_exp_f32 v251, v167\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v216, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "v_exp_f32 v250, v168\n" \
  "v_exp_f32 v251, v169\n" \
  "s_nop 0\n" \
  "v_cvt_pk_bf16_f32 v217, v250, v251\n" \
  "v_add_f32 v254, v254, v250\n" \
  "v_add_f32 v254, v254, v251\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_mask0_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_sub_u32 v255, s38, %[hi4]\n" \
  "v_mov_b32 v69, 0xff800000\n" \
  "v_cmp_ge_i32 vcc, 0, v255\n" \
  "v_cndmask_b32 v138, v138, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 1, v255\n" \
  "v_cndmask_b32 v139, v139, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 2, v255\n" \
  "v_cndmask_b32 v140, v140, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 3, v255\n" \
  "v_cndmask_b32 v141, v141, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 8, v255\n" \
  "v_cndmask_b32 v142, v142, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 9, v255\n" \
  "v_cndmask_b32 v143, v143, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 10, v255\n" \
  "v_cndmask_b32 v144, v144, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 11, v255\n" \
  "v_cndmask_b32 v145, v145, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 16, v255\n" \
  "v_cndmask_b32 v146, v146, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 17, v255\n" \
  "v_cndmask_b32 v147, v147, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 18, v255\n" \
  "v_cndmask_b32 v148, v148, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 19, v255\n" \
  "v_cndmask_b32 v149, v149, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 24, v255\n" \
  "v_cndmask_b32 v150, v150, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 25, v255\n" \
  "v_cndmask_b32 v151, v151, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 26, v255\n" \
  "v_cndmask_b32 v152, v152, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 27, v255\n" \
  "v_cndmask_b32 v153, v153, v69, vcc\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_mask1_%=:\n" \
  "s_nop 15\n" \
  "s_nop 3\n" \
  "v_sub_u32 v255, s38, %[hi4]\n" \
  "v_mov_b32 v69, 0xff800000\n" \
  "v_cmp_ge_i32 vcc, 0, v255\n" \
  "v_cndmask_b32 v154, v154, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 1, v255\n" \
  "v_cndmask_b32 v155, v155, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 2, v255\n" \
  "v_cndmask_b32 v156, v156, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 3, v255\n" \
  "v_cndmask_b32 v157, v157, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 8, v255\n" \
  "v_cndmask_b32 v158, v158, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 9, v255\n" \
  "v_cndmask_b32 v159, v159, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 10, v255\n" \
  "v_cndmask_b32 v160, v160, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 11, v255\n" \
  "v_cndmask_b32 v161, v161, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 16, v255\n" \
  "v_cndmask_b32 v162, v162, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 17, v255\n" \
  "v_cndmask_b32 v163, v163, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 18, v255\n" \
  "v_cndmask_b32 v164, v164, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 19, v255\n" \
  "v_cndmask_b32 v165, v165, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 24, v255\n" \
  "v_cndmask_b32 v166, v166, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 25, v255\n" \
  "v_cndmask_b32 v167, v167, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 26, v255\n" \
  "v_cndmask_b32 v168, v168, v69, vcc\n" \
  "v_cmp_ge_i32 vcc, 27, v255\n" \
  "v_cndmask_b32 v169, v169, v69, vcc\n" \
  "s_setpc_b64 s[44:45]\n" \
  ".Lfd2_end_%=:\n"
// clang-format on
#define FLASH_DP2_ASM_CLOBBERS_X \
  "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", \
  "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", \
  "v60", "v61", "v62", "v63", "v64", "v65", "v66", "v67", "v68", "v69", "v70", "v71", \
  "v72", "v73", "v74", "v75", "v76", "v77", "v78", "v79", "v80", "v81", "v82", "v83", \
  "v84", "v85", "v86", "v87", "v88", "v89", "v90", "v91", "v92", "v93", "v94", "v95", \
  "v96", "v97", "v98", "v99", "v100", "v101", "v102", "v103", "v104", "v105", "v106", "v107", \
  "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", \
  "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127", "v128", "v129", "v130", "v131", \
  "v132", "v133", "v134", "v135", "v136", "v137", "v138", "v139", "v140", "v141", "v142", "v143", \
  "v144", "v145", "v146", "v147", "v148", "v149", "v150", "v151", "v152", "v153", "v154", "v155", \
  "v156", "v157", "v158", "v159", "v160", "v161", "v162", "v163", "v164", "v165", "v166", "v167", \
  "v168", "v169", "v170", "v171", "v172", "v173", "v174", "v175", "v176", "v177", "v178", "v179", \
  "v180", "v181", "v182", "v183", "v184", "v185", "v186", "v187", "v188", "v189", "v190", "v191", \
  "v192", "v193", "v194", "v195", "v196", "v197", "v198", "v199", "v200", "v201", "v202", "v203", \
  "v204", "v205", "v206", "v207", "v208", "v209", "v210", "v211", "v212", "v213", "v214", "v215", \
  "v216", "v217", "v218", "v219", "v220", "v221", "v222", "v223", "v224", "v225", "v226", "v227", \
  "v228", "v229", "v230", "v231", "v232", "v233", "v234", "v235", "v236", "v237", "v238", "v239", \
  "v240", "v241", "v242", "v243", "v244", "v245", "v246", "v247", "v248", "v249", "v250", "v251", \
  "v252", "v253", "v254", "v255", "s36", "s37", "s38", "s39", "s40", "s41", "s42", "s43", \
  "s44", "s45", "vcc", "scc", "memory"
