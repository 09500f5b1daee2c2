// One level pass of k_search (pomcp_search.hip): the level of every lane that
// still descends.  Included into the kernel body twice, so that both forms share
// this text: in the generic kernel's loop (D = 0: the lane's depth is the
// runtime `depth`) and in the helper of the depth-specialised kernels' unrolled
// passes (D = 1..DL, a compile-time depth: every lane in the pass is at it).
// Expects D (constexpr int) and dc (DepthC<D>) in scope.
      if (phase == TP_LEVEL) {
        const uint4* const ap = reinterpret_cast<const uint4*>(an + (int64_t)blk * blk_bytes);
        const uint32_t j = take_mod(Env::kStepRange);
        const uint32_t ao = take_oth(s0, s1);
        PT_MARK(8);
        // the node line, prefetched by descend(): this arrival's N (its visits
        // + 1) and math.log(N) are in it
        // (D = 1 reads queue entry 0 itself, D > 1 never follows a START)
        if constexpr (D <= 1) {
          if (fw_on) {   // the line loaded before the previous backup's stores (q_flush)
            fw_on = false;
            if (blk == (D == 1 ? q_b[0] : fw_b)) {
              const uint32_t a4 = D == 1 ? q_a[0] : fw_a, v4 = D == 1 ? q_v[0] : fw_v;
              pre[0] = make_uint4(a4 == 0u ? v4 : pre[0].x, a4 == 1u ? v4 : pre[0].y,
                                  a4 == 2u ? v4 : pre[0].z, a4 == 3u ? v4 : pre[0].w);
              pre[1] = D == 1 ? q_s1[0] : fw_s1;
#pragma unroll
              for (int q = 2; q < kPre; ++q)
                pre[q] = sel4(q == part_vt((int)a4), D == 1 ? q_vt[0] : fw_vt, pre[q]);
            }
          }
        }
        nvis = (int)pre[1].y + 1;
        const double log_n = hilo_d(pre[1].z, pre[1].w);
        const double lnx = logtab(nvis + 1);   // written back by the backup (no wait here)
        uint4 st[kMaxA];   // {visits, -, value} per action, as select_action reads them
  #pragma unroll
        for (int q = 0; q < kMaxA; ++q)
          st[q] = q < A ? make_uint4(line_visits(pre[0], pre[1], q), 0u, pre[part_vt(q)].x,
                                     pre[part_vt(q)].y)
                        : make_uint4(0, 0, 0, 0);
        double lap[kMaxA];   // TM: the node's action_probs (its prior line)
#pragma unroll
        for (int q = 0; q < kMaxA; ++q)
          lap[q] = TM != 0 ? hilo_d(q & 1 ? ppr[q >> 1].z : ppr[q >> 1].x, q & 1 ? ppr[q >> 1].w : ppr[q >> 1].y)
                           : 0.0;
        PT_MARK(1);
        const int a = select_action(st, nvis, log_n, lap);
        PT_MARK(2);
        uint4 sa = st[0], va = pre[part_vt(0)];
  #pragma unroll
        for (int q = 1; q < kMaxA; ++q) {
          sa = sel4(q == a, st[q], sa);
          va = sel4(q == a, pre[part_vt(q < A ? q : 0)], va);
        }
        // the chosen action's child slots (second round trip) -- except for a
        // child beyond the depth / step limits (mcts.py:315): the simulation
        // stops there whatever its slot holds, so its record is deferred
        // (pomcp_device.h: no slot read or write; the re-root materialises the
        // children that survive it).  TM looks it up: the node's prior moves
        // on arrivals at existing children (potmmcp.py:255-264).
        // (p.defer = 0, pomcp_set_defer_cutoff: the eager lookup -- cheaper re-roots)
        // (D > 0: the depth half is a compile-time value -- the last pass is
        // always a cut-off level, an earlier one only by its particle's step)
        const bool cutc = (D > 0 ? D + 1 > DL : depth + 1 > p.depth_limit) || t + 1 > p.step_limit;   // mcts.py:315
        c_cut += cutc ? 1 : 0;   // (stats: n_cutoff, and n_deferred when deferring)
        const bool skipc = TM == 0 && p.defer && cutc;
        // An unrolled pass above the last one loads the slot line for every
        // lane: a lane that skips reads the slot line of its own block and
        // action (a valid address) and never uses it -- the skipc arm below
        // comes first -- so neither the zero fill nor the exec-mask block
        // round the loads is needed there.
#ifdef PB_NO_UNCOND_SLOTS   // A/B builds: zero fill and conditional loads in every pass
        constexpr bool kLoadAll = false;
#else
        constexpr bool kLoadAll = D > 0 && D < DL;
#endif
        uint4 sl[kSlots];
        if constexpr (kLoadAll) {
  #pragma unroll
          for (int q = 0; q < kSlots; ++q) sl[q] = ap[part_slot(a, q)];
        } else {
  #pragma unroll
          for (int q = 0; q < kSlots; ++q) sl[q] = make_uint4(0, 0, 0, 0);
          if (!skipc) {
  #pragma unroll
            for (int q = 0; q < kSlots; ++q) sl[q] = ap[part_slot(a, q)];
          }
        }
        PT_MARK(3);
        append();   // the previous level's record, after this level's loads
        uint32_t n0, n1;
        double r;
        int done;
        uint64_t okey;
        tree_step(a, ao, j, &n0, &n1, &r, &done, &okey, !skipc);
        bool match = false;
        int ks = 0;
        // An unrolled pass above the last one looks up whatever skipc says (a
        // skipping lane's result is not read: the skipc arm below comes
        // first): find_slot stays straight-line, and only a lane at
        // its step limit skips there.  At the last pass (D = DL: skipc is
        // wave-uniform) and in the generic loop, where whole waves skip, the
        // condition stays and the lookup is jumped over.
        if ((D > 0 && D < DL) || !skipc) ks = find_slot(sl, okey, &match);
        PT_MARK(12);
        const uint32_t ani = (uint32_t)(blk * A + a);
        uint32_t cid = 0;
        int cblk = -1, cvis = 1, ccode = epol + 1, existed = 0;
        leaf_rc = -1;
        if (skipc) {
          cid = p.cut_base + ani;
        } else if (ks >= 0) {
          uint4 sk = sl[0];
  #pragma unroll
          for (int q = 1; q < kSlots; ++q)
            sk = sel4(q == ks, sl[q], sk);
          cblk = match ? (int)sk.z : cblk;   // (selects, as at the root level)
          cvis = match ? (int)sk.w + 1 : cvis;
          n_nodes += match ? 0 : 1;
          existed = match ? 1 : 0;
          uint64_t nk = okey | kValidBit | ((uint64_t)done << 63);
          if constexpr (TM != 0) {
            ccode = match ? (int)((sk.y >> (kCodeShift - 32)) & 15u) : ccode;
            nk |= (uint64_t)ccode << kCodeShift;
          }
          uint4* slot = const_cast<uint4*>(ap) + part_slot(a, ks);
          // the slot changes beyond its visit count, or its count is needed
          // (no block yet, within the limits): pomcp_device.h
          const bool flip = (sk.y >> 31) != (uint32_t)done;
          if (!match || flip || (cblk < 0 && (done || !cutc)))
            *slot = make_uint4((uint32_t)nk, (uint32_t)(nk >> 32), (uint32_t)cblk, (uint32_t)cvis);
          if (match && cblk >= 0 && done) bump_node(cblk);
          cid = ani * kSlots + (uint32_t)ks + 1u;
          leaf_ptr = reinterpret_cast<int32_t*>(slot) + 2;
        } else {
          const OvfChild o = ovf_child(ani, okey, done, cblk, cvis, ccode);
          cid = o.cid;
          cblk = o.cblk;
          cvis = o.cvis;
          ccode = o.code;
          existed = o.existed;
          leaf_ptr = o.cptr;
          if (cblk >= 0 && done) bump_node(cblk);
        }
        if constexpr (TM != 0) {
          if (existed) {   // this node's action_probs move (potmmcp.py:255-264)
            prior_ema(lap, nvis);
            double* const pl = reinterpret_cast<double*>(const_cast<uint4*>(ap) + part_prior(A));
#pragma unroll
            for (int q = 0; q < kMaxA; ++q)
              if (q < A) pl[q] = lap[q];
          }
        }
        PT_MARK(13);
        if (err != 0 || PB_LOG_FULL() || (D > 0 ? false : plen >= kMaxPath)) {
          if (err == 0) err = POMCP_E_ARENA;
          phase = TP_DONE;
        } else {
          rec = LogRec{cid | ((uint32_t)lane << kIdBits), n0, n1};   // mcts.py:371
          app = true;
          PB_LOG_TAKE();
          const uint32_t ba = ((uint32_t)blk << 3) | (uint32_t)a;   // blk < 2^26 / 30
          push_path(dc, PathEntry{
              make_uint4(ba | ((uint32_t)done << 31), sa.x, (uint32_t)__double2loint(r),
                         (uint32_t)__double2hiint(r)),
              va,
              make_uint4(pre[1].x, (uint32_t)nvis, (uint32_t)__double2loint(lnx),
                         (uint32_t)__double2hiint(lnx))});
          PT_MARK(14);
          descend(DepthC<(D > 0 ? D + 1 : 0)>{}, done, cblk, cvis, n0, n1, ccode);
        }
        PT_MARK(4);
      }
