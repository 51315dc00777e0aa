// Body of the mv.Recalculate kernel, included INSIDE recalc_kernel and recalc_fdct_kernel (mvx_analyse_kernel.h) with MVX_RECALC_GEO set to the
// build's geometry type: the text of both kernels, not a function they call, so that the dct 1..4 build leaves the other's code exactly as it was.
// In scope: BPS, smem, Pp, Rp, jobs, ldsRow, ldsHist, histBins.
    const AParams &P = *Pp;
    const RParams &R = *Rp;
    const AJob &J = jobs[blockIdx.y];
    typedef Searcher<BPS, MVX_RECALC_GEO> S_t;
    S_t S(P, J);
    S.lds = (lds_u8 *)smem; S.ldsRow = ldsRow; S.ldsHist = ldsHist; S.histBins = histBins;
    if constexpr (S_t::FDCT) S.ldsDct = ldsHist + histBins * 4 + 64;
    S.blockSync = 0;
    for (int i = 0; i < 16; i++) S.prof[i] = 0;
    const int l = lane_id();
    S.setup_geometry(0);
    const int nBlk = S.nBlkX * S.nBlkY, b = blockIdx.x;
    const int valid = J.valid && ((const int *)J.oldBlob)[1] == 1; // MVRecalculate.c:152 fgopIsValid && reference frame inside the clip
    if (b == 0 && l == 0) { int *hdr = (int *)J.blob; hdr[0] = P.blobSize; hdr[1] = valid; }
    if (!valid) { // gopWriteDefaultToArray
        if (l == 0) { Vec d; d.x = 0; d.y = 0; d.sad = P.verybigSAD; S_t::st_vec(&S.vectors[b], d); }
        return;
    }
    S.smallestPlane = 0;
    S.blky = b / S.nBlkX; S.blkx = b - S.blky * S.nBlkX; S.blkIdx = b; S.blkScanDir = 1;
    const int stepX = P.blkX - P.ovX, stepY = P.blkY - P.ovY;
    S.x0 = S.hpad + stepX * S.blkx; S.y0 = S.vpad + stepY * S.blky;
    S.cx0 = S.chpad + (stepX >> S.logxr) * S.blkx; S.cy0 = S.cvpad + (stepY >> S.logyr) * S.blky;
    for (int t = l; t < S.TT; t += WAVE) { // source block -> LDS
        int loff, cb;
        gl_u8 *g = S.src_item_ptr(t, S.blkx, S.blky, stepX, stepY, loff, cb);
        A4x32 a = ld_chunk_g(g, cb);
        st_chunk_l(S.lds + loff, a, cb);
    }
    __builtin_amdgcn_wave_barrier();
    S.searchType = P.searchType; S.nSearchParam = P.nSearchParam; S.tryMany = 0;
    S.penaltyNew = P.pnew; S.penaltyZero = 0; S.pglobal = 0; S.badcount = 0; S.badrange = 0; S.badSAD = 0; S.LSAD = 0;
    S.dctmode = P.dctmode; S.dctweight16 = 8; S.sumLumaChange = 0; S.srcLuma = 0; // :1167
    S.zeroMVfieldShifted.x = 0; S.zeroMVfieldShifted.y = 0; S.zeroMVfieldShifted.sad = 0;
    S.globalMVPredictor.x = 0; S.globalMVPredictor.y = 0; S.globalMVPredictor.sad = 9999999;
    const int nLambdaLevel = P.lambda / (S.pel * S.pel);
    S.nLambda = S.blky == 0 ? 0 : nLambdaLevel;
    S.nDxMax = (S.pw - S.x0 - S.blkW) << S.logPel; // :1262-1265
    S.nDyMax = (S.ph - S.y0 - S.blkH) << S.logPel;
    S.nDxMin = -(S.x0 << S.logPel);
    S.nDyMin = -(S.y0 << S.logPel);
    // old vectors around the new block's centre (:1268-1321); plane headers walked like fgopUpdate
    const unsigned char *po = J.oldBlob + 8;
    for (int i = R.nLvCount - 1; i >= 1; i--) po += *(const int *)po;
    GL_AS const GVec *ov = (GL_AS const GVec *)(po + 4);
    const int centerX = P.blkX / 2 + stepX * S.blkx, blkxold = (centerX - R.blkX / 2) / R.stepX;
    const int centerY = P.blkY / 2 + stepY * S.blky, blkyold = (centerY - R.blkY / 2) / R.stepY;
    const int deltaX = max(0, centerX - (R.blkX / 2 + R.stepX * blkxold)), deltaY = max(0, centerY - (R.blkY / 2 + R.stepY * blkyold));
    const int x1 = min(R.nBlkX - 1, max(0, blkxold)), x2 = min(R.nBlkX - 1, max(0, blkxold + 1));
    const int y1 = min(R.nBlkY - 1, max(0, blkyold)), y2 = min(R.nBlkY - 1, max(0, blkyold + 1));
    Vec vo;
    if (R.smooth == 1) {
        const Vec v1 = S_t::ld_vec(&ov[x1 + y1 * R.nBlkX]), v2 = S_t::ld_vec(&ov[x2 + y1 * R.nBlkX]), v3 = S_t::ld_vec(&ov[x1 + y2 * R.nBlkX]), v4 = S_t::ld_vec(&ov[x2 + y2 * R.nBlkX]);
        const int ax = v1.x * R.stepX + deltaX * (v2.x - v1.x), ay = v1.y * R.stepX + deltaX * (v2.y - v1.y);
        const long long as = v1.sad * R.stepX + deltaX * (v2.sad - v1.sad);
        const int bx = v3.x * R.stepX + deltaX * (v4.x - v3.x), by = v3.y * R.stepX + deltaX * (v4.y - v3.y);
        const long long bs = v3.sad * R.stepX + deltaX * (v4.sad - v3.sad);
        vo.x = (ax + deltaY * (bx - ax) / R.stepY) / R.stepX;
        vo.y = (ay + deltaY * (by - ay) / R.stepY) / R.stepX;
        vo.sad = (as + deltaY * (bs - as) / R.stepY) / R.stepX;
    } else {
        const bool rx = deltaX * 2 >= R.stepX, ry = deltaY * 2 >= R.stepY;
        vo = S_t::ld_vec(&ov[(rx ? x2 : x1) + (ry ? y2 : y1) * R.nBlkX]);
    }
    vo = uni(vo);
    vo.x = (vo.x << S.logPel) >> R.logPel;
    vo.y = (vo.y << S.logPel) >> R.logPel;
    S.predictor = S.clip_mv(vo);
    S.predictor.sad = vo.sad * (P.blkX * P.blkY) / (R.blkX * R.blkY);
    S.bestMV = S.predictor;
    if (S.dctmode == 7 || S.dctmode == 8 || S.dctmode == 10 || (S_t::FDCT && S.dctmode >= 3)) S.srcLuma = S.src_luma();
    if constexpr (S_t::FDCT) { S.fdct_load_tables(); S.fdct_source(); }
    unsigned aL = 0, aC = 0;
    S.eval_cand(l, 6, S.predictor.x, S.predictor.y, S.predictor.y, aL, aC);
    aL = group_sum(aL, 6); aC = group_sum(aC, 6);
    if constexpr (S_t::FDCT) aL = S.fdct_apply(true, l, 6, S.predictor.x, S.predictor.y, aL);
    else if (S.dctmode != 0) aL = S.apply_dct(true, l, 6, S.predictor.x, S.predictor.y, aL);
    const long long sad = uni((long long)aL + (S.chroma ? (long long)aC : 0));
    S.bestMV.sad = sad;
    S.nMinCost = sad;
    if (sad > R.thSAD) S.search_block(2);
    if (l == 0) S_t::st_vec(&S.vectors[b], S.bestMV);
