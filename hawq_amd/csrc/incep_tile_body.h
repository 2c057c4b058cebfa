// The workgroup body of the LDS-tiled InceptionV3 conv (the method: incep_tiled.hip), from the tile constants to the closing brace of
// the epilogue.  A fragment, not a header: incep_tiled.hip, incep_group.hip and incep_fan.hip include it once each as the last
// statements of a function template (it returns from that function); incep_tile.h says why it is shared as text.  It expects
//   BM, BN, WPX, WCH, KS            the tile's template constants
//   a, Ho, Wo                       the conv's argument block (hawq_incep_conv_args, wave-uniform) and its output map
//   lds                             2 * (BM + BN) * 64 bytes of LDS, 16-byte aligned: the two stages
//   pblock, cblock                  the workgroup computes pixels pblock .. pblock + BM - 1 (long long) and channels cblock ..
//                                   cblock + BN - 1 (int): in scope, or defined by
//   INCEP_TILE_BLOCK                a macro, expanded once after P: empty where the includer got pblock and cblock from its caller,
//                                   their definitions where it works them out itself (incep_tiled_kernel: from there, and not from in
//                                   front of the fragment, the kernel compiles to the code it had with the body written out)
//   INCEP_TILE_STORED(p, cb, q)     a macro, expanded as a statement after a lane has stored the requantised channels cb .. cb + 15 of
//                                   pixel p, with what it stored in int q[16]: the hook of the fan-out epilogue, empty otherwise (a RAW
//                                   epilogue does not reach it)
    constexpr int NT = 64 * WPX * WCH * KS, RSTEP = NT / 4;
    constexpr int WM = BM / WPX / 32, WN = BN / WCH / 32;
    constexpr int APT = BM / RSTEP, BPT = BN / RSTEP, RPT = APT + BPT;
    constexpr int STAGE = (BM + BN) * 64;
    static_assert(BM % RSTEP == 0 && BN % RSTEP == 0 && BM % (32 * WPX) == 0 && BN % (32 * WCH) == 0, "tile shape");
    static_assert(WM * WN > 1, "a wave owns more than one MFMA tile");
    static_assert(KS == 1 || (KS == 2 && WM * WN * 16 * 64 * 4 * WPX * WCH <= 2 * STAGE), "K-split reduction must fit the stages");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, h = lane >> 5;
    const int wk = wave / (WPX * WCH), wr = wave % (WPX * WCH), wpx = wr % WPX, wch = wr / WPX;
    const int slot = tid & 3, r0 = tid >> 2;
    const long long P = (long long)a.N * Ho * Wo;
    INCEP_TILE_BLOCK
    const int C16 = a.Cin >> 4, K16 = a.KH * a.KW * C16, steps = (K16 + 3) >> 2;
    const int8_t *in = (const int8_t *)a.in, *wgt = (const int8_t *)a.wgt;

    // the rows this thread stages
    const int8_t *abase[APT];
    int iy0[APT], ix0[APT];
#pragma unroll
    for (int i = 0; i < APT; ++i) {
        const long long p = pblock + r0 + i * RSTEP;
        abase[i] = in, iy0[i] = -(1 << 20), ix0[i] = 0;   // a row beyond P: every tap fails the bounds test below
        if (p < P) {
            const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
            abase[i] = in + (size_t)(p / ((long long)Wo * Ho)) * a.H * a.W * a.Cin;
            iy0[i] = oy * a.stride - a.pad_h, ix0[i] = ox * a.stride - a.pad_w;
        }
    }
    const int8_t *wrow[BPT];
    bool wv[BPT];
#pragma unroll
    for (int j = 0; j < BPT; ++j) {
        const int q = r0 + j * RSTEP, co = cblock + (q & ~31) + cperm(q & 31);
        wv[j] = co < a.Cout;
        wrow[j] = wgt + (wv[j] ? (size_t)co * K16 * 16 : 0);
    }
    // this thread's k16 unit of the step to load next
    int k16 = slot, c16 = k16 % C16, kw = (k16 / C16) % a.KW, kh = (k16 / C16) / a.KW;

    v4i rg[RPT];
    bool ok[RPT];
    const v4i zero = {0, 0, 0, 0};
    // loads are unconditional (a refused element reads the first bytes of its operand) and zeroed when they are written to LDS:
    // no branch around a load, so all RPT of them are in flight together
    auto load = [&]() {
        const bool kv = k16 < K16;
#pragma unroll
        for (int i = 0; i < APT; ++i) {
            const int iy = iy0[i] + kh, ix = ix0[i] + kw;
            ok[i] = kv && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const size_t off = ok[i] ? ((size_t)iy * a.W + ix) * a.Cin + c16 * 16 : 0;
            rg[i] = *reinterpret_cast<const v4i *>((ok[i] ? abase[i] : in) + off);
        }
#pragma unroll
        for (int j = 0; j < BPT; ++j) {
            ok[APT + j] = kv && wv[j];
            rg[APT + j] = *reinterpret_cast<const v4i *>(wrow[j] + (ok[APT + j] ? (size_t)k16 * 16 : 0));
        }
        k16 += 4, c16 += 4;
        while (c16 >= C16) {
            c16 -= C16;
            if (++kw == a.KW) kw = 0, ++kh;
        }
    };
    auto write = [&](int stage) {
        char *s = lds + stage * STAGE;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            *reinterpret_cast<v4i *>(s + lds_off(r0 + i * RSTEP, slot)) = ok[i] ? rg[i] : zero;
        }
    };

    v16i acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    auto compute = [&](int stage) {
        const char *s = lds + stage * STAGE;
#pragma unroll
        for (int t = 0; t < 2 / KS; ++t) {
            const int kk = KS == 2 ? wk : t;   // the 32-byte half of the step
            v4i af[WM], bf[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i)
                af[i] = *reinterpret_cast<const v4i *>(s + lds_off(wpx * 32 * WM + 32 * i + l31, 2 * kk + h));
#pragma unroll
            for (int j = 0; j < WN; ++j)
                bf[j] = *reinterpret_cast<const v4i *>(s + lds_off(BM + wch * 32 * WN + 32 * j + l31, 2 * kk + h));
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(bf[j], af[i], acc[i][j], 0, 0, 0);
        }
    };

    load();
    write(0);
    __syncthreads();
    for (int s = 0; s < steps; ++s) {
        const bool more = s + 1 < steps;
        if (more) load();          // in flight under the MFMAs of step s
        compute(s & 1);
        if (more) write((s + 1) & 1);   // the other stage: last read in step s - 1, before the barrier that ended it
        __syncthreads();
    }

    if (KS == 2) {   // every wave is past the last barrier: the stages are free
        int *red = reinterpret_cast<int *>(lds);
        if (wk == 1) {
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[(((i * WN + j) * 16 + r) * (WPX * WCH) + wr) * 64 + lane] = acc[i][j][r];
        }
        __syncthreads();
        if (wk == 1) return;
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += red[(((i * WN + j) * 16 + r) * (WPX * WCH) + wr) * 64 + lane];
    }

    // acc[i][j][r] = channel cblock + 32 (wch WN + j) + 16 h + r of pixel pblock + 32 (wpx WM + i) + l31
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long long p = pblock + 32 * (wpx * WM + i) + l31;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int cb = cblock + 32 * (wch * WN + j) + 16 * h;
            if (p >= P || cb >= a.Cout) continue;   // Cout % 16 == 0: the 16 channels of a lane half are all valid or all not
            const size_t row = (size_t)p * a.ldo + a.c_off + cb;   // a multiple of 16 elements (hawq_incep_conv_tile_ok)
            int q[16];
            if (a.epilogue == HAWQ_INCEP_RAW) {
#pragma unroll
                for (int r = 0; r < 16; ++r) q[r] = acc[i][j][r] + a.bias[cb + r];
                v4i *o = reinterpret_cast<v4i *>((int32_t *)a.out + row);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = v4i{q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3]};
                continue;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cb + r;
                int v = acc[i][j][r] + a.bias[co];
                if (a.relu) v = max(v, 0);
                q[r] = clampi(dyadic_rne(v, a.m[co], a.ek[co]), a.q_lo, a.q_hi);
                if (a.epilogue == HAWQ_INCEP_REQUANT2) q[r] = clampi(dyadic_rne(q[r], a.m2, a.ek2), a.q2_lo, a.q2_hi);
            }
            if (a.out_bits == 16) {
                v4i *o = reinterpret_cast<v4i *>((int16_t *)a.out + row);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    v4i d;
#pragma unroll
                    for (int e = 0; e < 4; ++e) d[e] = (q[8 * r + 2 * e] & 0xffff) | (int)((unsigned)q[8 * r + 2 * e + 1] << 16);
                    o[r] = d;
                }
            } else {
                v4i d;
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = (int)pack4_i8(q[4 * e], q[4 * e + 1], q[4 * e + 2], q[4 * e + 3]);
                *reinterpret_cast<v4i *>((int8_t *)a.out + row) = d;
            }
            INCEP_TILE_STORED(p, cb, q);
        }
    }
