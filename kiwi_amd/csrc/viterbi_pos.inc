// Position-step best-path search (k_pos_path) -- included by viterbi_kernel.hip inside its namespace(s), so that every compilation of the search
// (Knlm, typo, CoNgram, typo + CoNgram; not the SkipBigram ones) gets its own copy next to the general kernel k_best_path.
//
// What it is.  The general kernel sweeps the lattice node by node and decides everything about a node inside the loop: ~3 400 wave instructions per
// node for ~7 transitions (profiles/r01_b_pmc_summary_c2.json: as many scalar as vector instructions), which is what bounds it.  Two facts of the
// lattice cut that down:
//   * nodes that END at the same position have all their predecessors complete and do not feed each other (a predecessor ends where a node starts):
//     the sweep can advance one END POSITION per step -- 35 instead of 68 dependent steps per 40-jamo sentence, ~13 work items per step instead of ~7,
//     i.e. a 16-lane row that is mostly full;
//   * which candidates are evaluated, every node-level score term and the rule scorer's node-side inputs are functions of the lattice alone: k_expand_pos
//     (lattice_kernels.hip) writes them once per batch as packed records (PosRec) and a position table (PosDesc), so the loop only multiplies the records
//     by the incoming paths.
// A step (four chunks per wavefront, a 16-lane group each, all four in lock step): a group's lanes 0..m-1 look its m nodes' predecessor state
// ranges up (LDS ring), lanes 0..nRec-1 turn its records into item counts (paths x start states).  Then the WAVEFRONT packs the items of all four
// groups into its 64 lanes -- records in lane order, a round being the next up to 64 items whatever 16-lane rows a record falls in -- and scores them
// together, one per lane (side terms + LM walk): a position has ~13 items, so four of them fill one wavefront where four separate 16-lane rounds left
// a quarter of the lanes idle and every group waiting for the slowest group's second round (26 % of a step, profiles/r03_j_pos_phases_c2.txt).  The
// per-key winner of the reference's path container (BestPathContainer.hpp:279-483; a key never spans two candidates, and carries its record here)
// comes from segmented scans -- one pass per distinct key of a record, the segments being the records, scanned along the rows and carried across
// them; kept states stream to their group's arena in item order;
// back in the groups, pruning per (node, root) against the best socket-free score (PathEvaluator.hpp:475-511) is 15 rotations of the row and lanes
// 0..m-1 commit the nodes' state ranges.  The reference's fallbacks run inside the step: the retry without left-condition penalties, the second reading
// of all-partial forms, the z-coda / z-siot shortcut (records of their own), and the disconnected-lattice test as reachability bit sets over positions.
//
// What a step does not do: a lattice that really is disconnected (the node's unknown-word evaluation), more than 16 nodes or records at a position, a
// record of more than PBIG_CAP items, a medium / large path container (> 128 live incoming paths), predecessors older than the LDS ring of nodes, a full
// arena or staging area.  The group then stops BEFORE the position (nothing of it is committed) and the chunk goes on in the general search at that node
// -- same arena, same per-node tables: for the first WorkView::posContSlots chunks of a launch inside this kernel (continueChunk below), for any further
// ones in k_best_path, launched after it (DevChunkResult::pad = node | reason << 24; kPosChunkDone = searched to the end; WorkView::posHandOver stays 0
// when nothing is left, and k_best_path then returns at once).  Results are the general kernel's bit for bit: same work items, same fp32 operations in
// the same order, same first-wins tie rule; the emulator suite and the GPU suite run both paths against the oracle and against each other on whole
// corpora (KAMD_POS_PATH=0 switches this kernel off).
#if !defined(KAMD_SBG) && !defined(KAMD_CONGG)
	// The lane-group width G is 16 (four chunks per wavefront; the round-3 kernel) or 8 (eight chunks per wavefront, round 5): the bookkeeping of a step --
	// table entry, predecessor ranges, pruning, retries, flags, commit -- costs the wavefront the same instructions whether its groups are 16 or 8 lanes
	// wide, and a position has 2 nodes and 3.4 records on average (more than 8 records in 0.9 % of the steps: a second pass), so eight groups halve that
	// cost per position; the items of eight positions (~ 116) also fill the rounds of 64 lanes better than those of four (~ 58, of which a round of four
	// 16-lane rows took 37 on average).  The LDS of a group shrinks with it (fewer staged records / new states / ring states), so that the wavefronts per
	// CU stay what they were and the chunks in flight double.
	template<int G> struct PosCaps
	{
#ifdef KAMD_TEST_SMALL_CAPS
		static constexpr uint32_t PST_CAP = 8;        // new states of one position staged in LDS for pruning / node bookkeeping
#else
		static constexpr uint32_t PST_CAP = G == 16 ? 64 : 32;
#endif
		static constexpr uint32_t PHR = G == 16 ? 32 : 16;      // most recent states whose hot quad (+ typo cost[, context id]) is kept in LDS: what a following step reads of a state
	};
	constexpr uint32_t PBIG_CAP = 64;      // items of one record beyond which the position is handed over (a round is one wavefront of items, and a record is never split over two rounds)
	// what the lanes that score a group's items need of the group (its lane 0 keeps it current in LDS): 16 dwords
	struct PosGroupCtx { uint64_t st, recs, uniq, nodeTypo; uint32_t stCap, stTop, posStart, ringTop, chunk, retry, ofNodes, nNodes; };
	static_assert(sizeof(PosGroupCtx) == 64, "PosGroupCtx");
	template<int G> struct PosLayT
	{
		static constexpr uint32_t PST_CAP = PosCaps<G>::PST_CAP, PHR = PosCaps<G>::PHR;
		static constexpr uint32_t RBEG = 0, REND = 4 * RING, RCUM = 8 * RING;      // as the general kernel's ring: first state / end / running live total of the last RING nodes
		static constexpr uint32_t NCNT = 12 * RING;                                   // u32[G]: per node of the position -- states | own-candidate states << 8 | live << 16 | live socket-free << 24
		static constexpr uint32_t ACUR = NCNT + 4 * G, ALAST = ACUR + 32, ATMP = ALAST + 32; // u32[8] each: reachable flags per position as bit sets (see the kernel)
		// u32[8], 16-lane groups only (the 8-lane build has no LDS left: it enumerates all parents): the dead flags of the most recent 256 states as a bit set (bit =
		// state index mod 256), written -- set or cleared -- for every new state where the pruning loop decides it; what lets a record enumerate LIVE parents only
		// (-DKAMD_TEST_DEAD_WINDOW=32: a test build of the lane emulator that looks 32 states back, so that its runs take the walk through the arena that a
		// longer range falls back to)
#ifdef KAMD_TEST_DEAD_WINDOW
		static constexpr uint32_t DWIN_BITS = KAMD_TEST_DEAD_WINDOW;
#else
		static constexpr uint32_t DWIN_BITS = 256;
#endif
		static constexpr uint32_t DWIN = ATMP + 32, DWIN_WORDS = DWIN_BITS / 32;
		static constexpr uint32_t GCTX = DWIN + (G == 16 ? 32 : 0);                   // PosGroupCtx
		static constexpr uint32_t RINFO = GCTX + 64;                                  // u32[G]: per record of the pass -- first incoming state | start states << 27 ... see the kernel
		static constexpr uint32_t PBEST = RINFO;                                      // f32[G], after the rounds (the records' entries are dead then): per node of the position the best socket-free score of the common root (pruning)
		static constexpr uint32_t OVFL = RINFO + 4 * G;                               // u32: a state of this group did not fit (arena / staging)
		static constexpr uint32_t RECS = OVFL + 16;                                   // PosRec[G]: the records of the pass (fetched by the group's lanes early in the step, read by whichever lanes score their items)
		static constexpr uint32_t STSC = RECS + G * 48;                               // f32[PST_CAP]
		static constexpr uint32_t STB = STSC + 4 * PST_CAP;                           // u16[PST_CAP]: StageBits | node-in-position << 8 | PSB_PASS1
		static constexpr uint32_t HOTR = (STB + 2 * PST_CAP + 15) & ~15u;             // uint4[PHR]: hot quads of the last PHR states (slot = state index mod PHR)
		static constexpr uint32_t TYPR = HOTR + 16 * PHR;                             // f32[PHR]: their accumulated typo cost
#ifdef KAMD_CONG
		static constexpr uint32_t CTXR = TYPR + 4 * PHR, SIZE = (CTXR + 4 * PHR + 15) & ~15u;   // u32[PHR]: their context id
#else
		static constexpr uint32_t CHR = TYPR + 4 * PHR, SIZE = (CHR + 8 * PHR + 15) & ~15u;     // u32[2 * PHR]: the next two nodes of their LM node's back-off chain (ModelView::lmChain)
#endif
		// shared by the wavefront: per lane of a round that a record's FIRST item takes (the lane of the record | this lane << 6) + 1, else 0;
		// after the steps (G == 8): the list of the chunks that go on in the general search
		static constexpr uint32_t ROWMAP = (64 / G) * SIZE, TOTAL = ROWMAP + 128;
	};
#if defined(KAMD_TYPO)
	constexpr uint32_t kPosLds16 = kPosKernelLdsBytes + 4 * kTypoRingExtra, kPosLds8 = kPosKernelLdsBytes8 + 8 * kTypoRingExtra;      // (what the engine launches these compilations with)
#else
	constexpr uint32_t kPosLds16 = kPosKernelLdsBytes, kPosLds8 = kPosKernelLdsBytes8;
#endif
	static_assert(PosLayT<16>::TOTAL <= kPosLds16 && PosLayT<8>::TOTAL <= kPosLds8, "k_pos_path LDS");
	static_assert(Lay<16>::TOTAL <= kPosLds16 && Lay<16>::TOTAL <= kPosLds8, "k_pos_path LDS: the general search carrying on in the kernel");
	enum : uint32_t { PSB_PASS1 = 0x1000 };
	// developer statistics of a host (lane-emulated) build with -DKAMD_POSSTATS: how full the rounds of k_pos_path are, printed at exit
#if defined(KAMD_POSSTATS) && defined(KAMD_HIPEMU)
	struct PosStats { std::atomic<unsigned long long> c[24]; ~PosStats() { fprintf(stderr, "[posstats] waveSteps %llu groupSteps %llu rounds %llu bigRecords %llu itemLanes %llu deadParents %llu scored %llu kept %llu multiChunkItems %llu roundsWithMulti %llu argmaxIters %llu reps %llu lmCalls %llu retries %llu rowsUsed %llu zItems %llu sockItems %llu testSteps %llu testChunks %llu straddled %llu arenaSelects %llu roundsPerStep %.4f\n",
		c[0].load(), c[1].load(), c[2].load(), c[3].load(), c[4].load(), c[5].load(), c[6].load(), c[7].load(), c[8].load(), c[9].load(), c[10].load(), c[11].load(), c[12].load(), c[13].load(), c[14].load(), c[15].load(), c[16].load(), c[17].load(), c[18].load(), c[19].load(), c[20].load(), c[0].load() ? (double)c[2].load() / (double)c[0].load() : 0.0); } };
	static PosStats gPosStats;
	struct PosHist { std::atomic<unsigned long long> h[6][70]; ~PosHist() { static const char* nm[6] = { "nRec", "nodes", "newStates", "itemsPerRecord", "parentAge", "nodeDist" }; for (int a = 0; a < 6; ++a) { fprintf(stderr, "[poshist] %s:", nm[a]); for (int b = 0; b < 70; ++b) if (h[a][b].load()) fprintf(stderr, " %d:%llu", b, h[a][b].load()); fprintf(stderr, "\n"); } } };
	static PosHist gPosHist;
#define PHIST(a, v) gPosHist.h[a][(v) < 69u ? (v) : 69u]++;
#define PSTAT(k, n) gPosStats.c[k] += (n);
#else
#define PSTAT(k, n) (void)0;
#define PHIST(a, v) (void)0;
#endif

	__device__ __forceinline__ uint32_t rowOr16(uint32_t v) { v |= rowRor<8>(v); v |= rowRor<4>(v); v |= rowRor<2>(v); v |= rowRor<1>(v); return v; }
	__device__ __forceinline__ uint32_t rowMaxU16(uint32_t v)
	{
		uint32_t o;
		o = rowRor<8>(v); v = o > v ? o : v; o = rowRor<4>(v); v = o > v ? o : v; o = rowRor<2>(v); v = o > v ? o : v; o = rowRor<1>(v); v = o > v ? o : v;
		return v;
	}
	__device__ __forceinline__ void ldsAdd(LDS_AS uint32_t* p, uint32_t v)      // ds_add_u32 (no return value)
	{
#if defined(__HIP_DEVICE_COMPILE__)
		__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
		__atomic_fetch_add((uint32_t*)p, v, __ATOMIC_RELAXED);
#endif
	}
	__device__ __forceinline__ void ldsOr(LDS_AS uint32_t* p, uint32_t v)      // ds_or_b32 (no return value)
	{
#if defined(__HIP_DEVICE_COMPILE__)
		__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
		__atomic_fetch_or((uint32_t*)p, v, __ATOMIC_RELAXED);
#endif
	}
	// inclusive prefix sum over the 16 lanes of a row (gl = lane in row)
	__device__ __forceinline__ uint32_t rowScan16(uint32_t v, uint32_t gl)
	{
		uint32_t t;
		t = rowRor<1>(v); v += gl >= 1 ? t : 0u; t = rowRor<2>(v); v += gl >= 2 ? t : 0u; t = rowRor<4>(v); v += gl >= 4 ? t : 0u; t = rowRor<8>(v); v += gl >= 8 ? t : 0u;
		return v;
	}
	// the same over the G lanes of a lane group (gl = lane in group; a lane never takes what a rotation brings in from outside its group)
	template<int G> __device__ __forceinline__ uint32_t grpScan(uint32_t v, uint32_t gl)
	{
		uint32_t t;
		t = rowRor<1>(v); v += gl >= 1 ? t : 0u; t = rowRor<2>(v); v += gl >= 2 ? t : 0u; t = rowRor<4>(v); v += gl >= 4 ? t : 0u;
		if constexpr (G == 16) { t = rowRor<8>(v); v += gl >= 8 ? t : 0u; }
		return v;
	}
	template<int G> __device__ __forceinline__ uint32_t grpOr(uint32_t v)
	{
		if constexpr (G == 16) return rowOr16(v);
		else { v |= __shfl_xor(v, 4, 8); v |= __shfl_xor(v, 2, 8); v |= __shfl_xor(v, 1, 8); return v; }
	}
	template<int G> __device__ __forceinline__ uint32_t grpMaxU(uint32_t v)
	{
		if constexpr (G == 16) return rowMaxU16(v);
		else { uint32_t o; o = __shfl_xor(v, 4, 8); v = o > v ? o : v; o = __shfl_xor(v, 2, 8); v = o > v ? o : v; o = __shfl_xor(v, 1, 8); v = o > v ? o : v; return v; }
	}
	__device__ __forceinline__ void ldsAnd(LDS_AS uint32_t* p, uint32_t v)      // ds_and_b32 (no return value)
	{
#if defined(__HIP_DEVICE_COMPILE__)
		__hip_atomic_fetch_and(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
		__atomic_fetch_and((uint32_t*)p, v, __ATOMIC_RELAXED);
#endif
	}
	// position of the k-th (from 0) set bit of v (v has more than k set bits): five popcounts
	__device__ __forceinline__ uint32_t nthSetBit(uint32_t v, uint32_t k)
	{
		uint32_t pos = 0, c;
		c = (uint32_t)__popc(v & 0xFFFFu); if (k >= c) { k -= c; pos += 16; v >>= 16; }
		c = (uint32_t)__popc(v & 0xFFu); if (k >= c) { k -= c; pos += 8; v >>= 8; }
		c = (uint32_t)__popc(v & 0xFu); if (k >= c) { k -= c; pos += 4; v >>= 4; }
		c = (uint32_t)__popc(v & 0x3u); if (k >= c) { k -= c; pos += 2; v >>= 2; }
		if (k >= (v & 1u)) pos += 1;
		return pos;
	}
	__device__ __forceinline__ void ldsMaxF(LDS_AS float* p, float v)      // ds_max_f32 (no return value)
	{
#if defined(__HIP_DEVICE_COMPILE__)
		__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
#else
		uint32_t o = __atomic_load_n((uint32_t*)p, __ATOMIC_RELAXED);
		while (v > __uint_as_float(o) && !__atomic_compare_exchange_n((uint32_t*)p, &o, __float_as_uint(v), false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
#endif
	}

	// The general search (searchChunk) for a chunk the position steps leave at node `stopAt & 0xFFFFFF`, called by k_pos_path itself (see the end of the kernel).
	// A real function: inlined, the general search's code cost the position steps a tenth of their speed (the registers and spills of a kernel are
	// allocated as a whole).  It reads the kernel's arguments where they are -- the kernarg segment, through scalar loads, like a kernel does -- instead
	// of taking them as parameters: copies on the caller's stack would be 1.2 KB of scratch memory per LANE of every wave of the launch.  PosKernArgs
	// restates k_pos_path's parameter list (every member is 8-byte aligned, so the argument layout is the struct layout); the scratch pointer handed in
	// beside it is compared with the one found there, and a mismatch leaves the chunk to k_best_path.
	struct PosKernArgs { ModelView M; BatchView B; WorkView W; SearchParams P; const uint32_t* chunkOrder; uint32_t nWork; TYPO_ONLY(const float* nodeTypoAll;) CONG_ONLY(CongDev CG;) };
#ifdef KAMD_HIPEMU
	__device__ __noinline__ void continueChunk(const PosKernArgs* A, uint32_t chunk, uint32_t gl, uint32_t grp, uint32_t slot, uint32_t stopAt, const uint8_t* scratchCheck, const uint32_t* orderCheck, uint32_t nWorkCheck)
	{
#else
	__device__ __noinline__ void continueChunk(uint32_t chunk, uint32_t gl, uint32_t grp, uint32_t slot, uint32_t stopAt, const uint8_t* scratchCheck, const uint32_t* orderCheck, uint32_t nWorkCheck)
	{
		// (a callable function is not handed the kernarg segment pointer itself -- the intrinsic folds to null there -- but the pointer to the hidden
		// arguments, which follow the explicit ones at the next 8-byte boundary; the loads below stay scalar loads)
		const PosKernArgs* A = (const PosKernArgs*)((const uint8_t*)__builtin_amdgcn_implicitarg_ptr() - ((sizeof(PosKernArgs) + 7) & ~(size_t)7));
#endif
		// (the layout assumption is checked on a member of the middle AND the two members behind the structs: a change that moves only the tail is caught too)
		// (it also leaves the chunk's result word -- searched to the end here | why it left the position steps, or still to be searched by k_best_path --, so that
		// the kernel keeps nothing in registers over the call)
		if (A->W.posScratch != scratchCheck || A->chunkOrder != orderCheck || A->nWork != nWorkCheck)
		{
			if (gl == 0) { A->W.results[chunk].pad = stopAt; *A->W.posHandOver = 1; }
			return;
		}
		const ModelView& M = A->M; const SearchParams& P = A->P; const BatchView& B = A->B; const WorkView& W = A->W;
		CONG_ONLY(const CongDev& CG = A->CG;)
		GroupCtx<16> X(M, P);
		X.gl = gl; X.gshift = grp * 16; X.lds = grp * Lay<16>::SIZE;
		X.scratch = reinterpret_cast<GroupScratch*>(W.posScratch) + slot;
		X.tl = nullptr;
		TYPO_ONLY(X.typoAll = A->nodeTypoAll; X.nodeTypo = nullptr;)
		CONG_ONLY(X.CG = &CG; X.outFirst = false;)
		searchChunk<16>(X, B, W, chunk, stopAt & 0xFFFFFFu);
		if (gl == 0) W.results[chunk].pad = kPosChunkDone | (stopAt & 0xFF000000u);      // (bits 24..31: why it left the position steps, developer statistics)
	}

	template<int G, int WPS>
	__global__ void __launch_bounds__(64, WPS) k_pos_path(ModelView M, BatchView B, WorkView W, SearchParams P, const uint32_t* chunkOrder, uint32_t nWork TYPO_ONLY(, const float* nodeTypoAll) CONG_ONLY(, CongDev CGv))
	{
		static_assert(G == 16 || G == 8, "a lane group is one DPP row or half of one");
		using PosLay = PosLayT<G>;
		constexpr uint32_t NG = 64 / G, GM = (1u << G) - 1u, PST_CAP = PosLay::PST_CAP, PHR = PosLay::PHR;
		// Records enumerate the LIVE states of their predecessor range only (16-lane groups): an item of a pruned parent would load it, find it dead and leave --
		// 15 % of the item lanes of the benchmark corpus.  A dead parent contributes to no output and the live ones keep their order, so nothing else changes.
		constexpr bool kLiveOnly = G == 16;
		// passes of G records a position's records go through: two for an 8-lane group (16 records, as in round 5); for a 16-lane group one -- and two in the typo
		// compilations (32 records: the alternatives of a typo bring many candidates to one place; 8 of c5's 8 192 chunks had such a position and finished in the
		// general search, 0.3 ms behind everything else)
#ifdef KAMD_TYPO
		constexpr uint32_t kP = 2;
#else
		constexpr uint32_t kP = 16 / G;
#endif
		// gl / grp: lane in its group / the group (the bookkeeping of a step).  The ITEMS of a round sit in the four 16-lane DPP rows of the wavefront whatever
		// the group width is: il / irow = lane in its row / the row.
		const uint32_t lane = threadIdx.x, gl = lane & (uint32_t)(G - 1), gshift = lane & (uint32_t)(64 - G), grp = lane / (uint32_t)G, lds = grp * PosLay::SIZE;
		const uint32_t il = lane & 15u, irow = lane >> 4;
		LDS_AS uint32_t* rBeg = ldsPtr<uint32_t>(lds + PosLay::RBEG);
		LDS_AS uint32_t* rEnd = ldsPtr<uint32_t>(lds + PosLay::REND);
		LDS_AS uint32_t* rCum = ldsPtr<uint32_t>(lds + PosLay::RCUM);
		LDS_AS uint32_t* nCnt = ldsPtr<uint32_t>(lds + PosLay::NCNT);
		LDS_AS uint32_t* aCur = ldsPtr<uint32_t>(lds + PosLay::ACUR);
		LDS_AS uint32_t* aLast = ldsPtr<uint32_t>(lds + PosLay::ALAST);
		LDS_AS uint32_t* aTmp = ldsPtr<uint32_t>(lds + PosLay::ATMP);
		LDS_AS uint32_t* gctx = ldsPtr<uint32_t>(lds + PosLay::GCTX);
		LDS_AS uint32_t* rinfo = ldsPtr<uint32_t>(lds + PosLay::RINFO);
		LDS_AS uint32_t* ovfL = ldsPtr<uint32_t>(lds + PosLay::OVFL);
		LDS_AS uint16_t* rowMap = ldsPtr<uint16_t>(PosLay::ROWMAP);
		rowMap[lane] = 0;      // (all clear between rounds: a round's item lanes clear what its records marked)
		// (bit x of a set; every lane of the group writes the same word, so no lane waits for another's store)
		auto tbit = [](LDS_AS uint32_t* a, uint32_t x) -> uint32_t { return (a[(x >> 5) & 7u] >> (x & 31u)) & 1u; };
		auto sbit = [](LDS_AS uint32_t* a, uint32_t x) { a[(x >> 5) & 7u] |= 1u << (x & 31u); };
		LDS_AS float* typR = ldsPtr<float>(lds + PosLay::TYPR);
#ifdef KAMD_CONG
		LDS_AS uint32_t* ctxR = ldsPtr<uint32_t>(lds + PosLay::CTXR);
#else
		LDS_AS uint32_t* chR = ldsPtr<uint32_t>(lds + PosLay::CHR);
#endif
		const uint32_t hotR = lds + PosLay::HOTR;
		LDS_AS float* stSc = ldsPtr<float>(lds + PosLay::STSC);
		LDS_AS uint16_t* stB = ldsPtr<uint16_t>(lds + PosLay::STB);
#define GBALLOT(p) ((uint32_t)((__ballot(p) >> gshift) & GM))
#define GSHFL(v, l) __shfl((v), (int)(l), G)
		// whole-wavefront ballot / shuffle, and the cross-lane operations of the item rounds (16-lane rows whatever the group width) -- the lane emulator of
		// tests/hipemu keeps a lane group as this kernel's convergence width: it needs to be told what all 64 lanes do together
#ifdef KAMD_HIPEMU
#define WBALLOT(p) hipemu_ballot64(p)
#define WSHFL(v, l) hipemu_shfl64((v), (int)(l))
#define WREADLANE(v, l) hipemu_shfl64((v), (int)(l))
#define IROR(N, v) ((uint32_t)hipemu_row_ror64((int)(v), (N)))
#define IRORF(N, v) __uint_as_float((uint32_t)hipemu_row_ror64((int)__float_as_uint(v), (N)))
#else
#define WBALLOT(p) ((unsigned long long)__ballot(p))
#define WSHFL(v, l) __shfl((v), (int)(l), 64)
#define WREADLANE(v, l) ((uint32_t)__builtin_amdgcn_readlane((int)(v), (int)(l)))      // the source lane is the same for the whole wavefront: v_readlane_b32, no LDS round trip
#define IROR(N, v) rowRor<N>(v)
#define IRORF(N, v) rowRorF<N>(v)
#endif
		// developer aid (KAMD_POS_DEBUG builds + KAMD_HANGDUMP=1): where a lane group is, readable from the host while the kernel runs
#ifdef KAMD_POS_DEBUG
#define PBEACON(code, a, b2, c2) { if (W.beacon && mine && gl == 0) { uint32_t* bq_ = W.beacon + 64ull * chunk; __builtin_nontemporal_store((uint32_t)(code), bq_); __builtin_nontemporal_store((uint32_t)(a), bq_ + 1); __builtin_nontemporal_store((uint32_t)(b2), bq_ + 2); __builtin_nontemporal_store((uint32_t)(c2), bq_ + 3); } }
		unsigned long long tlLast = clock64(); uint32_t tlAcc[14] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#define PTL(k) { const unsigned long long t_ = clock64(); tlAcc[k] += (uint32_t)(t_ - tlLast); tlLast = t_; }
#else
#define PBEACON(code, a, b2, c2)
#define PTL(k)
#endif
		// s_waitcnt vmcnt(0), stated where the loads in flight have arrived on every path that does work -- the compiler then knows so on the other paths too.
		// The operand in the gfx9-family encoding: vmcnt = bits 3:0 and 15:14 (0: wait for all), expcnt = bits 6:4 and lgkmcnt = bits 11:8 at their maxima (7, 15:
		// no wait).  On gfx950 vmcnt counts the wave's vector STORES as well as its loads, in issue order: the wait also drains whatever the wave has stored
		// before it (before the loop: the start node; behind the group phase: nothing of this step yet -- a step's state stores are issued in its rounds and
		// behind them -- but what the previous step stored, which the wait for this step's records would cover anyway).
		constexpr int kWaitVm0 = (0 << 0) | (0 << 14) | (7 << 4) | (15 << 8);
#if defined(__HIP_DEVICE_COMPILE__)
#define POS_LOADS_ARRIVED() __builtin_amdgcn_s_waitcnt(kWaitVm0)
#else
#define POS_LOADS_ARRIVED() (void)0
#endif
		const unsigned long long lowerMask64 = (1ull << lane) - 1ull;

		// One chunk per lane group, four per block, no work loop (with one, the hipcc of ROCm 7.2 produced gfx950 code whose outermost back edge never
		// came round on the hardware: profiles/r03_c_hang_beacons.txt).  Blocks are scheduled longest chunk first (chunkOrder).  The four groups step
		// through their lattices TOGETHER: a group without work left (no chunk, handed over, finished) stays in the loop and lends its lanes.
		const uint32_t ci = blockIdx.x * NG + grp;
		const bool mine = ci < nWork;
		const uint32_t chunk = mine ? chunkOrder[ci] : chunkOrder[0];
		bool active = mine && W.results[chunk].status == CS_OK;
		if (mine && !active && gl == 0) W.results[chunk].nPaths = 0;
		const bool searching = active;      // this group has a lattice to search (for the epilogue)
		PBEACON(1, ci, 0, 0)
		const uint32_t nBase = W.nodeBase[chunk];
		const uint32_t Gn = W.nNodes[chunk];
		const uint32_t stCap = (uint32_t)(W.stateBase[chunk + 1] - W.stateBase[chunk]);
		// A chunk's tables are a kernel argument plus the chunk's offset.  Over the step loop a lane keeps the 32-bit offsets only -- nBase for the per-node tables,
		// recBase for the records -- and an address is formed where it is used, against the wave-uniform base: a dozen pointers held per lane were 24 VGPRs
		// for the whole loop, and at three waves per SIMD the step paid for them with scratch reloads (the one of `recs` at its very head, in front of the
		// records' loads).  The arena, the start states and the nodes' typo costs are written to the group's PosGroupCtx once, here: the lanes that score items
		// read them there anyway, and so does the group itself (stArena) where it needs the arena inside the loop.
		// (nodeLive: the chunk's two 16-bit slots per node of WorkView::tmpIdx, of which the live counts take the first Gn -- element 2 * nBase + i, as the
		// general search reads them when it takes a chunk over)
		const uint32_t recBase = W.packBase[chunk];
		auto nodeStOff = [&](uint32_t i) -> uint32_t& { return W.nodeStateOff[nBase + i]; };
		auto nodeStCnt = [&](uint32_t i) -> uint32_t& { return W.nodeStateCnt[nBase + i]; };
		auto nodeLive = [&](uint32_t i) -> uint16_t& { return W.tmpIdx[2ull * nBase + i]; };
		auto reach = [&](uint32_t i) -> uint8_t& { return W.reach[nBase + i]; };
		auto desc = [&](uint32_t i) -> const PosDesc& { return W.posDesc[nBase + i]; };
		auto posPrev = [&](uint32_t i) -> const uint32_t& { return W.posPrev[nBase + i]; };
		auto posStarts = [&](uint32_t i) -> const uint32_t& { return W.posMask[nBase + i]; };
		auto recs = [&](uint32_t i) -> const PosRec& { return W.posRecs[recBase + i]; };
		auto stArena = [&]() -> DevState* { return reinterpret_cast<DevState*>(((LDS_AS uint64_t*)gctx)[0]); };
		auto uniqStates = [&]() -> const uint8_t* { return reinterpret_cast<const uint8_t*>(((LDS_AS uint64_t*)gctx)[2]); };
		const uint32_t nPos = active ? desc(0).firstRec : 0u, eosStart = active ? desc(0).pad2 : 0u;      // positions; the position the end node's predecessors end at
		TYPO_ONLY(const uint32_t nBase2 = nBase + W.nodeBase[B.nChunks];)      // (start positions five to eight of a position: lattices over typo graphs, k_expand_pos)
		// The reference's `reachable` flags (PathEvaluator.hpp:1159-1176, 1286-1299) as bit sets over positions (LDS, up to 256 positions): aCur -- some
		// node ending at the position carries a set flag now; aLast -- the flags the last disconnected-lattice test left behind (it rewrites the flag of
		// every later node by propagation; a formless node never sets its own afterwards, so it keeps that value).  A node's predecessors all end at
		// one position, so the propagation runs over positions: reachable(x) <=> one of the (<= 4 distinct) start positions of x's nodes is reachable.
		const bool canPropagate = nPos <= 255 && active && desc(0).nNodes == 0;
		bool scanned = false;
		if (gl < 8) { aCur[gl] = gl == 0 ? 1u : 0u; aLast[gl] = 0; if constexpr (kLiveOnly) ldsPtr<uint32_t>(lds + PosLay::DWIN)[gl] = 0; }
		if (gl == 0)
		{
			LDS_AS uint64_t* g64 = (LDS_AS uint64_t*)gctx;
			for (uint32_t k = 8; k < 16; ++k) gctx[k] = 0;
			gctx[12] = chunk; gctx[15] = Gn;      // (the end of the search reads the chunk's index and node count back from here: whatever was formed from them above then ends before the loop)
			g64[0] = (uint64_t)(W.states + W.stateBase[chunk]); g64[1] = 0; g64[2] = (uint64_t)(B.spStates + B.spOff[chunk]);
#ifdef KAMD_TYPO
			g64[3] = (uint64_t)(nodeTypoAll + nBase);
#else
			g64[3] = 0;
#endif
		}
		rinfo[gl] = 0; if (gl == 0) *ovfL = 0;

		uint32_t stTop = 1, cumLive = 1;
		uint32_t ringTop = 1;      // highest arena slot + 1 ever written (a retry rewinds stTop, not what its discarded states overwrote in the ring)
		uint32_t stopAt = 0;       // node at which the general kernel takes over (0: not needed so far) | reason << 24 (developer statistics)
		if (active)
		{
			// start node (PathEvaluator.hpp:1224-1226)
			if (gl == 0)
			{
				const MorphRec m0 = M.morphs[0];
				DevState* st = W.states + W.stateBase[chunk];
				storeState(st, 0, M.h.bosNode, 0.f, 0.f, 0, m0.feat, COMMON_ROOT, 0, 0, m0.prevFlags, 0, 0xFFFFFFFFu, 0, 0.f, 0, 0);
				nodeStOff(0) = 0; nodeStCnt(0) = 1; nodeLive(0) = 1;
				rBeg[0] = 0; rEnd[0] = 1; rCum[0] = 1;
				ldsStore4(hotR, make_uint4((uint32_t)M.h.bosNode, 0u, (uint32_t)m0.feat | ((uint32_t)COMMON_ROOT << 16), (uint32_t)m0.prevFlags << 8));
				typR[0] = 0.f;
#ifdef KAMD_CONG
				ctxR[0] = 0;
#else
				const uint32_t c1 = M.lmChain[2 * (uint32_t)M.h.bosNode], c2 = M.lmChain[2 * (uint32_t)M.h.bosNode + 1];
				chR[0] = c1; chR[1] = c2;
				*reinterpret_cast<uint2*>(&st[0].pad0) = make_uint2(c1, c2);
#endif
			}
			for (uint32_t k = gl; k < Gn; k += G) reach(k) = k == 0 ? 1 : 0;
			if (!nPos) { stopAt = 1u | (8u << 24); active = false; }      // (no position program: the general kernel searches the chunk from its first node)
		}

		// The static side of a step -- its table entry, the nodes' predecessor ranges, the records' item multipliers -- is fetched one step ahead (the
		// table entry two): none of it is on the step's dependent chain then.  A = this step, B = the next one.
		uint4 dqA = make_uint4(0, 0, 0, 0), dqB = make_uint4(0, 0, 0, 0);
		uint32_t ppA = 0, rqA = 0;
		// (the build for two waves per SIMD has the registers to fetch the next step's RECORDS a step ahead as well: 12 dwords per record lane)
		uint4 recA0 = make_uint4(0, 0, 0, 0), recA1 = recA0, recA2 = recA0, recB0 = recA0, recB1 = recA0, recB2 = recA0;
		if (active)
		{
			dqA = *reinterpret_cast<const uint4*>(&desc(1));
			if (nPos >= 2) dqB = *reinterpret_cast<const uint4*>(&desc(2));
			if (gl < ((dqA.x >> 16) & 0xFFu)) ppA = posPrev((dqA.x & 0xFFFFu) + gl);
			if (gl < (dqA.z & 0xFFFFu)) rqA = recs(dqA.y + gl).rq;
			if constexpr (WPS <= 2) if (gl < (dqA.z & 0xFFFFu)) { const uint4* rp0 = reinterpret_cast<const uint4*>(&recs(dqA.y + gl)); recA0 = rp0[0]; recA1 = rp0[1]; recA2 = rp0[2]; }
		}

		// attempt 0: form conditions on.  A node whose own candidates yield no state is evaluated again with the conditions turned into a penalty
		// (attempt 1: retry0, PathEvaluator.hpp:468-473); a node still without any state whose form also has the unknown-noun reading gets the same
		// for that reading (attempt 2: retry1, the second evaluation's own retry :1277-1287).  A retry redoes the whole position: nothing of it is committed.
		uint32_t pi = 1, attempt = 0, retry0 = 0, retry1 = 0;
		uint4 dqC = make_uint4(0, 0, 0, 0); uint32_t ppB = 0, rqB = 0;      // (fetched in a step's first attempt, kept over its retries)
		uint32_t guardSteps = 0;
		// (what was fetched above has arrived before the first step: a wait for it inside the loop would be a wait for everything the step has in flight -- the
		// counter retires in order, and the compiler cannot tell how many of a step's conditional loads stand behind a load from before the loop)
		POS_LOADS_ARRIVED();
		__syncthreads();

		while (WBALLOT(active))
		{
			if (++guardSteps > 4u * 0x10000u) break;      // (belt and braces: a step advances or retries at most twice; a wavefront that did spin would hang the GPU)
			if (lane == 0) PSTAT(0, 1)
			if (gl == 0 && active) PSTAT(1, 1)
			// ================= the groups, each for itself: what this step's position is made of =================
			const uint4 dq = dqA;
			const uint32_t i0 = dq.x & 0xFFFFu, m = (dq.x >> 16) & 0xFFu, firstRec = dq.y, nRec = dq.z & 0xFFFFu;
			// the records of a position (<= 16) go through the rounds in passes of G: one pass for a 16-lane group, a second one for an 8-lane group with more than 8
			uint32_t Qp[kP]; uint32_t rqp[kP], pBegRp[kP];
#pragma unroll
			for (uint32_t ps_ = 0; ps_ < kP; ++ps_) { Qp[ps_] = 0; rqp[ps_] = 0; pBegRp[ps_] = 0; }
			uint32_t posStart = stTop;
			CONG_ONLY(uint32_t ofNodes = 0;)      // bit j: node j's incoming paths satisfy the m condition (below)
			uint4 rec0 = recA0, rec1 = recA1, rec2 = recA2;      // (the records of the first pass: fetched a step ahead, or in flight while the group does its bookkeeping)
			if (active)
			{
				PBEACON(2, pi, i0, (m << 16) | nRec)
				PTL(0)
				if ((dq.x >> 24) || m > (uint32_t)G || nRec > kP * (uint32_t)G) { stopAt = i0 | (1u << 24); active = false; }      // (flagged by k_expand_pos, or more nodes / records than this instantiation's passes take)
			}
			if (active)
			{
				// (three waves per SIMD: this step's records are the first loads of the step -- the memory counter retires in order, so the wait for them, at the
				// end of the group's bookkeeping, leaves the fetches for the later steps behind them in flight)
				if constexpr (WPS > 2) if (gl < nRec) { const uint4* rp0 = reinterpret_cast<const uint4*>(&recs(firstRec + gl)); rec0 = rp0[0]; rec1 = rp0[1]; rec2 = rp0[2]; }
				rqp[0] = rqA;
				if constexpr (kP > 1) if (nRec > (uint32_t)G && gl + G < nRec) rqp[kP - 1] = recs(firstRec + G + gl).rq;      // (a second pass: fetched here, off the first pass's chain)
				if (!attempt)
				{
					dqC = make_uint4(0, 0, 0, 0); ppB = 0; rqB = 0;
					if (pi + 2 <= nPos) dqC = *reinterpret_cast<const uint4*>(&desc(pi + 2));
					if (pi + 1 <= nPos)
					{
						if (gl < ((dqB.x >> 16) & 0xFFu)) ppB = posPrev((dqB.x & 0xFFFFu) + gl);
						if (gl < (dqB.z & 0xFFFFu)) rqB = recs(dqB.y + gl).rq;
						if constexpr (WPS <= 2) if (gl < (dqB.z & 0xFFFFu)) { const uint4* rp0 = reinterpret_cast<const uint4*>(&recs(dqB.y + gl)); recB0 = rp0[0]; recB1 = rp0[1]; recB2 = rp0[2]; }
					}
				}
				// ---- nodes of the position (lane j = node i0 + j): incoming state range and live count from the ring ----
				uint32_t pBeg = 0, nP = 0, nLv = 0; bool bad = false; uint32_t why = 0;      // (nLv: the live ones among the nP incoming states)
				if (gl < m)
				{
					const uint32_t fp = ppA & 0xFFFFu, lp = fp + ((ppA >> 16) & 0xFFu);
					if (i0 + gl - fp + 1 >= RING) { bad = true; why = 2; }      // (predecessors older than the ring: the general kernel reads the HBM tables)
					else
					{
						pBeg = rBeg[fp & (RING - 1)];
						nP = rEnd[lp & (RING - 1)] - pBeg;
						const uint32_t nLive = rCum[lp & (RING - 1)] - (fp ? rCum[(fp - 1) & (RING - 1)] : 0u);
						if (nLive > P.smallMax) { bad = true; why = 3; }      // medium / large path container (BestPathContainer.hpp:275-277)
						nLv = nLive;
					}
				}
				nCnt[gl] = 0;
				// ---- records (lane k of pass p = record firstRec + p * G + k): items = incoming paths x start states ----
				if (gl == 0) { PHIST(0, nRec) PHIST(1, m) }
#pragma unroll
				for (uint32_t ps_ = 0; ps_ < kP; ++ps_)
				{
					const uint32_t rq = rqp[ps_];
					const uint32_t nlR = (rq >> 8) & 0xFFu, Rr = rq & 0xFFu;
					const uint32_t nPk = GSHFL(kLiveOnly ? nLv : nP, nlR), pBegR = GSHFL(pBeg, nlR);
					const uint32_t Q = ps_ * G + gl < nRec ? nPk * Rr : 0u;
#if defined(KAMD_POSSTATS) && defined(KAMD_HIPEMU)
					{ const uint32_t nAll = GSHFL(nP, nlR); if (kLiveOnly && ps_ * G + gl < nRec && !bad) PSTAT(5, (nAll - nPk) * Rr) }
#endif
					if (Q > PBIG_CAP || pBegR >= (1u << 27)) { bad = true; why = 4; }
					Qp[ps_] = Q; pBegRp[ps_] = pBegR;
					if (ps_ * G + gl < nRec) PHIST(3, Q)
				}
				if (gl < m && !bad) PHIST(5, i0 + gl - (ppA & 0xFFFFu))
				if (GBALLOT(bad)) { stopAt = i0 | (grpMaxU<G>(why) << 24); active = false; }
#ifdef KAMD_CONG
				// Which kernel of the reference rounds the scores of an evaluation's regular candidates (DESIGN.md section 2): the specialised GEMV (output
				// scale first) iff they share one first word (PR_OUT_FIRST, static) and the live socket-free incoming paths carry m >= 4, m != 8 unique contexts
				if (active)
				{
					uint32_t wantL = 0;
#pragma unroll
					for (uint32_t ps_ = 0; ps_ < kP; ++ps_)
					{
						const uint32_t rq = rqp[ps_], nlR = (rq >> 8) & 0xFFu;
						const uint32_t nPk = GSHFL(nP, nlR);
						if (ps_ * G + gl < nRec && (rq & PR_OUT_FIRST) && nPk >= 4) wantL |= 1u << nlR;
					}
					const uint32_t want = grpOr<G>(wantL);
					const DevState* st = want ? stArena() : nullptr;
					for (uint32_t wn = want; wn; wn &= wn - 1)
					{
						const uint32_t j = (uint32_t)__ffs((int)wn) - 1u;
						const uint32_t pb = GSHFL(pBeg, j), np = GSHFL(nP, j);
						if (G < 16 || np > 16)
						{
							// more incoming paths than one row (<= PBIG_CAP: a larger node was handed over above; an 8-lane group always counts this way): their
							// contexts are listed in LDS -- in the record area, which this step fills only below -- and every path looks for its context among
							// the earlier ones
							static_assert(4 * PBIG_CAP <= G * 48, "context list in the record area");
							LDS_AS uint32_t* cxs = ldsPtr<uint32_t>(lds + PosLay::RECS);
							for (uint32_t b = 0; b < np; b += G)
							{
								const uint32_t k = b + gl;
								if (k < np) { const Hot h = loadHot(st, pb + k); cxs[k] = (!h.dead() && !h.socket()) ? st[pb + k].pad0 : 0xFFFFFFFFu; }
							}
							waveSyncLds();
							uint32_t mu = 0;
							for (uint32_t b = 0; b < np; b += G)
							{
								const uint32_t k = b + gl;
								bool isNew = false;
								if (k < np)
								{
									const uint32_t cx = cxs[k];
									isNew = cx != 0xFFFFFFFFu;
									for (uint32_t e = 0; isNew && e < k; ++e) isNew = cxs[e] != cx;
								}
								mu += (uint32_t)__popc(GBALLOT(isNew));
							}
							waveSyncLds();
							if (mu >= 4 && mu != 8) ofNodes |= 1u << j;
							continue;
						}
						if constexpr (G == 16)
						{
						uint32_t cx = 0xFFFFFFFFu; bool ok = false;
						if (gl < np) { const Hot h = loadHot(st, pb + gl); ok = !h.dead() && !h.socket(); cx = st[pb + gl].pad0; }
						const uint32_t okw = ok ? 1u : 0u;
						bool isNew = ok;
#define KAMD_UNIQ_STEP(N) { const uint32_t oc = rowRor<N>(cx), oo = rowRor<N>(okw); isNew = isNew & !((oo != 0) & (oc == cx) & (((gl - N) & 15u) < gl)); }
						KAMD_UNIQ_STEP(1) KAMD_UNIQ_STEP(2) KAMD_UNIQ_STEP(3) KAMD_UNIQ_STEP(4) KAMD_UNIQ_STEP(5) KAMD_UNIQ_STEP(6) KAMD_UNIQ_STEP(7) KAMD_UNIQ_STEP(8)
						KAMD_UNIQ_STEP(9) KAMD_UNIQ_STEP(10) KAMD_UNIQ_STEP(11) KAMD_UNIQ_STEP(12) KAMD_UNIQ_STEP(13) KAMD_UNIQ_STEP(14) KAMD_UNIQ_STEP(15)
#undef KAMD_UNIQ_STEP
						const uint32_t mu = (uint32_t)__popc(GBALLOT(isNew));
						if (mu >= 4 && mu != 8) ofNodes |= 1u << j;
						}
					}
				}
#endif
				if (active)
				{
					// what the lanes that will score this group's items need of it: per record the first incoming state and the start-state count; the group's pointers and counters
					rinfo[gl] = pBegRp[0] | ((rqp[0] & 0xFFu) << 27);
					if (gl < nRec) { ldsStore4(lds + PosLay::RECS + 48 * gl, rec0); ldsStore4(lds + PosLay::RECS + 48 * gl + 16, rec1); ldsStore4(lds + PosLay::RECS + 48 * gl + 32, rec2); }
					if (gl == 0)
					{
						gctx[8] = stCap; gctx[9] = stTop; gctx[10] = stTop; gctx[11] = ringTop; gctx[13] = retry0 | (retry1 << 16);
#ifdef KAMD_CONG
						gctx[14] = ofNodes;
#else
						gctx[14] = 0;
#endif
						*ovfL = 0;
					}
					posStart = stTop;
				}
				PTL(1)
			}
			// (three waves per SIMD: a group that stages its records has waited for them, and with them for the fetches issued behind them.  A group that stopped
			// above has not, and the head of the next step would wait there for everything in flight -- the state stores of this step among them -- before it
			// may reuse the registers)
			if constexpr (WPS > 2) POS_LOADS_ARRIVED();
			__syncthreads();

			for (uint32_t pass = 0; pass < kP; ++pass)
			{
			if (pass)
			{
				// ---- (8-lane groups) the records beyond the first G of a position: staged where the first pass's were, scored by the same rounds ----
				if (!WBALLOT(active && nRec > (uint32_t)G)) break;
				if (active)
				{
					rinfo[gl] = pBegRp[kP - 1] | ((rqp[kP - 1] & 0xFFu) << 27);
					if (G + gl < nRec)
					{
						const uint4* rp0 = reinterpret_cast<const uint4*>(&recs(firstRec + G + gl));
						ldsStore4(lds + PosLay::RECS + 48 * gl, rp0[0]); ldsStore4(lds + PosLay::RECS + 48 * gl + 16, rp0[1]); ldsStore4(lds + PosLay::RECS + 48 * gl + 32, rp0[2]);
					}
				}
				__syncthreads();
			}
			const uint32_t Qw = active ? ((kP > 1 && pass) ? Qp[kP - 1] : Qp[0]) : 0u;

			// ================= the wavefront: the items of all four positions, packed into its lanes =================
			// Records in lane order (group 0's, then group 1's ...).  A round is the next up to 64 items: the longest prefix of the remaining records whose
			// items fit the wavefront, one item per lane, whatever 16-lane rows a record falls in (a record has at most PBIG_CAP = 64 items, so it always fits).
			{
				uint32_t S16 = Qw;
				{ uint32_t t; t = IROR(1, S16); S16 += il >= 1 ? t : 0u; t = IROR(2, S16); S16 += il >= 2 ? t : 0u; t = IROR(4, S16); S16 += il >= 4 ? t : 0u; t = IROR(8, S16); S16 += il >= 8 ? t : 0u; }
				const uint32_t T0 = WREADLANE(S16, 15), T1 = WREADLANE(S16, 31), T2 = WREADLANE(S16, 47);
				const uint32_t Winc = S16 + (irow >= 1 ? T0 : 0u) + (irow >= 2 ? T1 : 0u) + (irow >= 3 ? T2 : 0u);      // inclusive prefix over the wavefront
				const unsigned long long nzAll = WBALLOT(Qw != 0);
				uint32_t recDoneW = 0, baseW = 0, guardW = 0;
				while (recDoneW < 64)
				{
					const unsigned long long nz = nzAll & ~((1ull << recDoneW) - 1ull);
					if (!nz) break;
					if (++guardW > 80u) { *ovfL = 1; break; }      // (belt and braces: every round takes at least one record)
					const bool take = lane >= recDoneW && Winc - baseW <= 64u;      // a prefix of the remaining records (Winc is non-decreasing; baseW = the items of the records done)
					const uint32_t n = (uint32_t)__popcll(WBALLOT(take));
					if (!n) { *ovfL = 1; break; }      // (cannot happen: the first remaining record has at most 64 items)
					const uint32_t nItems = WREADLANE(Winc, recDoneW + n - 1) - baseW;
					const uint32_t myStart = Winc - Qw - baseW;      // wavefront lane of this record's first item
					PTL(2)
					if (lane == 0) { PSTAT(2, 1) PSTAT(14, (nItems + 15u) >> 4) }
					if (take && Qw) { if (Qw > 16u) PSTAT(3, 1) if ((myStart >> 4) != ((myStart + Qw - 1u) >> 4)) PSTAT(19, 1) }
					// ---- item (= wavefront lane) -> its record's lane: every record marks the lane its FIRST item takes with (its lane | that lane << 6) + 1; an
					// item lane finds its record's mark by filling the marks forward -- along its row (four row steps), then across the rows from lanes 15, 31
					// and 47 (wave-uniform sources) --, leaves its entry cleared for the next round and fetches the item count from the record's lane ----
					if (take && Qw) rowMap[myStart] = (uint16_t)((lane | (myStart << 6)) + 1u);
					baseW += nItems; recDoneW += n;
					__syncthreads();
					bool valid = lane < nItems;
					uint32_t e = rowMap[lane];
					rowMap[lane] = 0;
					{ uint32_t o;
					  o = IROR(1, e); e = (e == 0 && il >= 1) ? o : e;
					  o = IROR(2, e); e = (e == 0 && il >= 2) ? o : e;
					  o = IROR(4, e); e = (e == 0 && il >= 4) ? o : e;
					  o = IROR(8, e); e = (e == 0 && il >= 8) ? o : e;
					  o = WREADLANE(e, 15); e = (e == 0 && irow == 1) ? o : e;
					  o = WREADLANE(e, 31); e = (e == 0 && irow == 2) ? o : e;
					  o = WREADLANE(e, 47); e = (e == 0 && irow == 3) ? o : e; }
					e = e ? e - 1u : 0u;
					const uint32_t recLane = valid ? (e & 63u) : lane;
					const uint32_t startK = valid ? (e >> 6) : lane;      // (lane of the record's first item)
					const uint32_t Qrec = WSHFL(Qw, recLane);
					const uint32_t lastK = valid ? startK + Qrec - 1u : lane;      // (lane of the record's last item: the record's later items may belong to the next row)
					const uint32_t local = lane - startK;
					// ---- the owner group's side ----
					const uint32_t owner = recLane / (uint32_t)G, k = recLane & (uint32_t)(G - 1), ldsO = owner * PosLay::SIZE;
					const uint4 g0 = ldsLoad4(ldsO + PosLay::GCTX), g1 = ldsLoad4(ldsO + PosLay::GCTX + 16), g2 = ldsLoad4(ldsO + PosLay::GCTX + 32), g3 = ldsLoad4(ldsO + PosLay::GCTX + 48);
					DevState* stO = reinterpret_cast<DevState*>((uint64_t)g0.x | ((uint64_t)g0.y << 32));
					const uint8_t* uniqO = reinterpret_cast<const uint8_t*>((uint64_t)g1.x | ((uint64_t)g1.y << 32));
					const float* nodeTypoO = reinterpret_cast<const float*>((uint64_t)g1.z | ((uint64_t)g1.w << 32)); (void)nodeTypoO;
					const uint32_t stCapO = g2.x, stTopO = g2.y, posStartO = g2.z, ringTopO = g2.w;
					const uint32_t retry0O = g3.y & 0xFFFFu, retry1O = g3.y >> 16;
					CONG_ONLY(const uint32_t ofNodesO = g3.z;)
					const uint32_t ri = ldsPtr<uint32_t>(ldsO + PosLay::RINFO)[k];
					const uint32_t pBegK = ri & 0x7FFFFFFu, R = ri >> 27;
					const uint32_t hotRO = ldsO + PosLay::HOTR;
					LDS_AS float* typRO = ldsPtr<float>(ldsO + PosLay::TYPR);
#ifdef KAMD_CONG
					LDS_AS uint32_t* ctxRO = ldsPtr<uint32_t>(ldsO + PosLay::CTXR);
#else
					LDS_AS uint32_t* chRO = ldsPtr<uint32_t>(ldsO + PosLay::CHR);
#endif
					LDS_AS float* stScO = ldsPtr<float>(ldsO + PosLay::STSC);
					LDS_AS uint16_t* stBO = ldsPtr<uint16_t>(ldsO + PosLay::STB);
					uint4 ra = make_uint4(0, 0, 0, 0), rb = ra, rc = ra;
					if (valid) { ra = ldsLoad4(ldsO + PosLay::RECS + 48 * k); rb = ldsLoad4(ldsO + PosLay::RECS + 48 * k + 16); rc = ldsLoad4(ldsO + PosLay::RECS + 48 * k + 32); }
					Cand c;
					c.firstWid = ra.x; c.secondWid = ra.y; c.chunkOff = ra.z; c.lastSeqId = ra.w;
					c.morph = rb.x; c.flagsFeat = rb.y; c.tagw = rb.z; c.cntw = rb.w;
					c.additional = __uint_as_float(rc.x); c.sbw = rc.z & 0xFFu; c.ruleBits = (rc.z >> 8) & 0xFFu; c.R = R;
					c.lmId = 0; c.userScore = 0; c.combinedId = 0; c.qOff = 0;
					const uint32_t nodeIdx = rc.y & 0xFFFFu; const uint16_t ownFeat = (uint16_t)(rc.y >> 16);
					const uint8_t ownKind = (uint8_t)(rc.z >> 16), nflags = (uint8_t)(rc.z >> 24);
					const uint32_t nl = (rc.w >> 8) & 0xFFu;
					const bool spaceBefore = nflags & NF_SPACE_BEFORE;
					const bool isZ = (rc.w & PR_Z) != 0;
					uint32_t p = local, r = 0;
					if (R > 1) { p = local / R; r = local % R; }      // R > 1 only for quote / sentence-break candidates under several start states

					PTL(3)
					float cand = 0, firstChunk = 0, rTypo = 0; int32_t lmNode = 0; uint8_t rootKey = 0, sp = 0;
					CONG_ONLY(uint32_t ctx = 0;)
					CONG_ONLY(uint32_t pctx = 0;)
#ifndef KAMD_CONG
					uint32_t pch1 = 0, pch2 = 0, nch1 = 0, nch2 = 0;      // back-off chain of the parent's LM node / of the item's new one
#endif
					if (valid) PSTAT(4, 1)
					// the parent: state pBegK + p -- or (live parents only) the p-th LIVE state from pBegK on, selected by popcounts over the owner group's dead-bit
					// window; a range that reaches behind the window (or bits a discarded attempt's states have overwritten: ringTop is the high-water mark) is
					// walked in the arena instead -- slow and rare
					uint32_t pidx = pBegK + p;
					if constexpr (kLiveOnly) if (valid)
					{
						uint32_t k = p;
						if (ringTopO - pBegK <= PosLay::DWIN_BITS)
						{
							LDS_AS uint32_t* dw = ldsPtr<uint32_t>(ldsO + PosLay::DWIN);
							uint32_t w = pBegK >> 5;
							uint32_t v = ~dw[w & (PosLay::DWIN_WORDS - 1u)] & (0xFFFFFFFFu << (pBegK & 31u));
							uint32_t c = (uint32_t)__popc(v);
							for (uint32_t it = 0; k >= c && it < PosLay::DWIN_WORDS; ++it) { k -= c; ++w; v = ~dw[w & (PosLay::DWIN_WORDS - 1u)]; c = (uint32_t)__popc(v); }
							pidx = k < c ? (w << 5) + nthSetBit(v, k) : pBegK;      // (k < c always: the record's item count is the range's live count)
						}
						else
						{
							PSTAT(20, 1)
							uint32_t idx = pBegK;
							for (; idx + 1 < posStartO; ++idx) { if (!loadHot(stO, idx).dead()) { if (!k) break; --k; } }
							pidx = idx;
						}
					}
					if (valid)
					{
						// what the step reads of its parent state: from the LDS ring of the last PHR states, else (older) from the arena
						const uint32_t slot = pidx & (PHR - 1);
						PHIST(4, ringTopO - pidx)
						Hot ps;
						if (ringTopO - pidx <= PHR)
						{
							const uint4 a = ldsLoad4(hotRO + 16 * slot);
							ps.lmNode = (int32_t)a.x; ps.accScore = __uint_as_float(a.y); ps.w2 = a.z; ps.w3 = a.w;
							rTypo = typRO[slot];
#ifdef KAMD_CONG
							pctx = ctxRO[slot];
#else
							pch1 = chRO[2 * slot]; pch2 = chRO[2 * slot + 1];
#endif
						}
						else
						{
							ps = loadHot(stO, pidx);
							rTypo = stO[pidx].accTypoCost;
#ifdef KAMD_CONG
							pctx = stO[pidx].pad0;
#else
							const uint2 pc = *reinterpret_cast<const uint2*>(&stO[pidx].pad0); pch1 = pc.x; pch2 = pc.y;
#endif
						}
						const bool single = c.single();
						const uint8_t ctag = c.tag(), csock = c.socket();
						uint32_t firstWid = c.firstWid; bool widReplaced = false;
#ifdef KAMD_POS_DEBUG
						if (ps.accScore == 12345.678f && c.additional == 9876.5f) tlAcc[0] += 1;      // (forces the parent data and the record to have arrived before the stamp)
						PTL(12)
#endif
						const float ignoreCondScore = ((((rc.w & PR_PASS1) ? retry1O : retry0O) >> nl) & 1u) ? -10.f : 0.f;
						CONG_ONLY(float icDeferred = 0;)
						do
						{
							if (ps.dead()) { if (!kLiveOnly) PSTAT(5, 1) valid = false; break; }
							if (isZ) PSTAT(15, 1)
							if (csock) PSTAT(16, 1)
							if (isZ)
							{
								// z-coda / z-siot shortcut (PathEvaluator.hpp:389-432): the path is copied iff its last morpheme's tag admits the shortcut
								const uint8_t lastTag = M.morphs[stO[pidx].wid].tag;
								if (!((uint8_t)c.secondWid == T_Z_CODA ? (isJClass(lastTag) || isEClass(lastTag)) : isNNClass(lastTag))) { valid = false; break; }
								cand = ps.accScore + c.additional * P.typoCostWeight;
								lmNode = (int32_t)local;      // (every copy is its own state: the key is the item)
								break;
							}
#ifdef KAMD_CONG
							if (!csock && (ps.leftFeat() & LF_PREV_ZSIOT) && (!isNNClass(ctag) || spaceBefore)) { valid = false; break; }
							if (csock && !single && !ps.socket()) { valid = false; break; }
							if (!(csock && !single) && ps.socket()) { valid = false; break; }
#else
							if ((ps.leftFeat() & LF_PREV_ZSIOT) && (!isNNClass(ctag) || spaceBefore)) { valid = false; break; }
#endif
							cand = ps.accScore + c.additional;
							firstChunk = c.additional;
							if (ps.socket())
							{
								if (ps.socket() != csock || single) { valid = false; break; }
								if (spaceBefore)
								{
									if (P.spaceTol > 0) cand -= P.spacePenalty; else { valid = false; break; }
								}
							}
#ifdef KAMD_CONG
							if (csock && !single) { firstWid = M.morphs[M.morphs[stO[pidx].wid].combinedId].lmId; widReplaced = true; }
#else
							if (csock && !single)
							{
								// the reference keeps the combined word id of the latest matching split stem for all later predecessors (PathEvaluator.hpp:578-591)
								for (uint32_t qi = pidx + 1; qi-- > pBegK; )
								{
									const Hot qs = loadHot(stO, qi);
									if (qs.dead() || !qs.socket() || qs.socket() != csock) continue;
									if ((qs.leftFeat() & LF_PREV_ZSIOT) && (!isNNClass(ctag) || spaceBefore)) continue;
									if (spaceBefore && !(P.spaceTol > 0)) continue;
									firstWid = M.morphs[M.morphs[stO[qi].wid].combinedId].lmId; widReplaced = true;
									break;
								}
							}
#endif
							// FormEvaluator (PathEvaluator.hpp:293-310)
							if (!(ps.leftFeat() & (LF_STR_SSC | LF_TAG_SSC)))
							{
								const bool ok = featTest(ps.leftFeat() & 0x1FFF, c.vowel(), c.polar());
#ifdef KAMD_CONG
								// a regular candidate gets the penalty AFTER its first LM score: ((acc + morphScore) + ll) + ignoreCondScore (CoNgramModel.cpp:163-168)
								if (ignoreCondScore != 0) { if (!csock) icDeferred = ok ? 0 : ignoreCondScore; else cand += ok ? 0 : ignoreCondScore; }
#else
								if (ignoreCondScore != 0) cand += ok ? 0 : ignoreCondScore;
#endif
								else if (!ok) { valid = false; break; }
							}
							lmNode = ps.lmNode;
							CONG_ONLY(ctx = pctx;)
							if (!(csock && single))
							{
								// prohibit <v> without <chunk> (PathEvaluator.hpp:604-608)
								if (widReplaced ? (M.morphs[firstWid].tag == T_P) : ((c.flags() & MF_FIRST_WID_IS_P) != 0)) { valid = false; break; }
#ifdef KAMD_CONG
								float ll = congStep(M, CGv, lmNode, ctx, firstWid, ((ofNodesO >> nl) & 1u) && (rc.w & PR_OUT_FIRST) && !csock);
								cand += ll; firstChunk += ll;
								cand += icDeferred;
#else
								float ll = lmProgressChain(M, lmNode, pch1, pch2, firstWid);
								cand += ll; firstChunk += ll;
								PSTAT(12, 1) PSTAT(6, 1)
								if (!single && c.nChunks() > 1) PSTAT(8, 1)
#endif
#ifdef KAMD_POS_DEBUG
								if (ll == 12345.678f) tlAcc[0] += 1;
								PTL(13)
#endif
								if (!single)
								{
									const uint32_t nCh = c.nChunks();
									for (uint32_t ch = 1; ch < nCh; ++ch)
									{
										const uint32_t wid = ch == 1 ? c.secondWid : M.chunkLm[c.chunkOff + ch];
										if ((c.flags() & MF_ANY_REST_WID_IS_P) && M.morphs[wid].tag == T_P) { valid = false; break; }
#ifdef KAMD_CONG
										ll = congStep(M, CGv, lmNode, ctx, wid, false);
#else
										// (the chain of the node the previous word led to: one more load, then all contexts of this word at once)
										const uint2 mc = *reinterpret_cast<const uint2*>(M.lmChain + 2 * (size_t)(uint32_t)lmNode);
										ll = lmProgressChain(M, lmNode, mc.x, mc.y, wid);
#endif
										cand += ll;
									}
									if (!valid) break;
								}
							}
#ifndef KAMD_CONG
							{ const uint2 nc = *reinterpret_cast<const uint2*>(M.lmChain + 2 * (size_t)(uint32_t)lmNode); nch1 = nc.x; nch2 = nc.y; }      // (needed by the states this item may become; in flight during the arg-max)
#endif
							// insertToPathContainer (PathEvaluator.hpp:193-251)
							sp = ps.spState();
							rootKey = ps.rootId();
							if (c.quoteOrBullet())
							{
								if (rootKey == COMMON_ROOT) sp = uniqO[r];
								else if (r != 0) { valid = false; break; }   // a path already bound to a root is inserted once
							}
							const float rs = ruleScore(c, ps.prevFlags(), sp);
							cand = cand + rs; firstChunk = firstChunk + rs;
							if (c.ruleBits & RB_DIALECT) { cand = cand - P.dialectCost; firstChunk = firstChunk - P.dialectCost; }
							sp = nextSpState(c, sp);
						} while (0);
					}
					PTL(4)
					if (valid) PSTAT(7, 1)
					// key: LM node | new special state | previous root | group and record
					const uint64_t rKey = valid ? ((uint64_t)(uint32_t)lmNode | ((uint64_t)sp << 32) | ((uint64_t)rootKey << 40) | ((uint64_t)recLane << 48)) : KINVALID;
					const float rScore = cand, rFcs = firstChunk;

					// writes the state of a key's winner -- item `wl` of this round's record k -- at arena slot `pos`
					// (wx1, wx2: CoNgram -- the winner's context id; Knlm -- the next two nodes of the new LM node's back-off chain)
					auto emitState = [&](uint32_t pos, bool ring, int32_t wNode, uint8_t wSp, uint8_t wRoot, float wscore, float wfcs, float wtyp, uint32_t wx1, uint32_t wx2, uint32_t wl, uint32_t parent)
					{
						const uint32_t rslot = pos & (PHR - 1);
						const uint32_t wr = R != 1 ? wl % R : 0u;
						const uint32_t rel = pos - posStartO;
						if (isZ)
						{
							// the copy of the parent with the shortcut's morpheme put on (its LM state, root, special state, socket, own form are handed on unchanged)
							const uint4* ps4 = reinterpret_cast<const uint4*>(stO + parent);
							const uint4 a = ps4[0], b2 = ps4[1], c2 = ps4[2];
							const uint16_t lfMorph = (uint16_t)c.chunkOff; const uint8_t nmPrevFlags = (uint8_t)(c.chunkOff >> 16); const bool newMorphSocket = (c.chunkOff >> 24) & 1u;
							const uint8_t pOwnKind = (uint8_t)(a.w >> 24), pSocket = (uint8_t)a.w, pRoot = (uint8_t)(a.z >> 16), pSp = (uint8_t)(a.z >> 24);
							const uint16_t pLf = (uint16_t)a.z;
							const uint16_t lf = pOwnKind ? (uint16_t)((pLf & (0x1FFF | LF_STR_SSC)) | (lfMorph & (LF_TAG_SSC | LF_PREV_ZSIOT))) : lfMorph;
							const float nscore = __uint_as_float(a.y) + c.additional * P.typoCostWeight;
							storeState(stO, pos, (int32_t)a.x, nscore, __uint_as_float(b2.x) - c.additional, c.firstWid, lf, pRoot, pSp, pSocket, nmPrevFlags, pOwnKind, parent, c.firstWid,
								__uint_as_float(c2.x), (uint16_t)nodeIdx, (uint16_t)(c2.y >> 16) STATE_EXTRA(, c2.z));
							if (ring)
							{
								ldsStore4(hotRO + 16 * rslot, make_uint4(a.x, __float_as_uint(nscore), (uint32_t)lf | ((uint32_t)pRoot << 16) | ((uint32_t)pSp << 24), (uint32_t)pSocket | ((uint32_t)nmPrevFlags << 8) | ((uint32_t)pOwnKind << 24)));
								typRO[rslot] = __uint_as_float(b2.x) - c.additional;
#ifdef KAMD_CONG
								ctxRO[rslot] = c2.z;
#else
								chRO[2 * rslot] = c2.z; chRO[2 * rslot + 1] = c2.w;
#endif
							}
#ifndef KAMD_CONG
							*reinterpret_cast<uint2*>(&stO[pos].pad0) = make_uint2(c2.z, c2.w);
#endif
							stScO[rel] = nscore;
							stBO[rel] = (uint16_t)((pRoot == COMMON_ROOT ? 0u : pRoot + 1u) | (newMorphSocket ? (uint32_t)SB_MORPH_SOCKET : 0u) | (pSocket ? (uint32_t)SB_STATE_SOCKET : 0u) | (nl << 8));
							return;
						}
#ifdef KAMD_TYPO
						const float wtypo = wtyp + nodeTypoO[nodeIdx];      // accTypoCost + node->typoCost (PathEvaluator.hpp:235)
#else
						const float wtypo = wtyp + 0.f;
#endif
#ifdef KAMD_POS_TRACE
						fprintf(stderr, "emit lane %u pos %u node %u parent %u wtyp %g nodeTypo %g wl %u R %u pBegK %u morph %u score %.9g lm %d\n", lane, pos, nodeIdx, parent, wtyp, (double)(wtypo - wtyp), wl, R, pBegK, c.morph, (double)wscore, wNode);
#endif
						const bool single = c.single();
						const uint8_t newRoot = (c.quoteOrBullet() && wRoot == COMMON_ROOT) ? (uint8_t)wr : wRoot;
						const uint8_t stSocket = single ? c.socket() : 0;
						const bool own = single && ownKind;
						const uint16_t lf = own ? (uint16_t)(ownFeat | (c.leftFeat() & (LF_TAG_SSC | LF_PREV_ZSIOT))) : c.leftFeat();
						storeState(stO, pos, wNode, wscore, wtypo, c.lastSeqId, lf, newRoot, wSp, stSocket, c.prevFlags(), own ? ownKind : 0, parent, c.morph, wfcs,
							(uint16_t)nodeIdx, own ? (uint16_t)nodeIdx : 0 CONG_ONLY(, wx1));
						if (ring)
						{
							ldsStore4(hotRO + 16 * rslot, make_uint4((uint32_t)wNode, __float_as_uint(wscore), (uint32_t)lf | ((uint32_t)newRoot << 16) | ((uint32_t)wSp << 24),
								(uint32_t)stSocket | ((uint32_t)c.prevFlags() << 8) | ((uint32_t)(own ? ownKind : 0) << 24)));
							typRO[rslot] = wtypo;
#ifdef KAMD_CONG
							ctxRO[rslot] = wx1;
#else
							chRO[2 * rslot] = wx1; chRO[2 * rslot + 1] = wx2;
#endif
						}
#ifdef KAMD_CONG
						(void)wx2;
#else
						*reinterpret_cast<uint2*>(&stO[pos].pad0) = make_uint2(wx1, wx2);
#endif
						stScO[rel] = wscore;
						stBO[rel] = (uint16_t)((newRoot == COMMON_ROOT ? 0u : newRoot + 1u) | (c.socket() ? (uint32_t)SB_MORPH_SOCKET : 0u) | (stSocket ? (uint32_t)SB_STATE_SOCKET : 0u)
							| (nl << 8) | ((rc.w & PR_PASS1) ? (uint32_t)PSB_PASS1 : 0u));
					};
					const uint32_t keyLo = (uint32_t)rKey, keyHi = (uint32_t)(rKey >> 32);
					bool rep; float best, wfcs, wtyp; uint32_t wl, wx1, wx2, wNodeU, wHi, wpar;
					{
						// ---- per key: its representative (the key's first item, which emits the state) and its winner (best score, first item on ties).
						// Items of one record that share a key are settled together: every record takes the key of its first unsettled item, the items
						// carrying it find their best by a segmented scan over the wavefront (segments = records: four steps along the row, then the pair at
						// the last lane of every row is carried into the lanes of the next row whose record began before it -- the lower lane wins on
						// equal scores throughout), and the representative fetches it from the record's last lane.  One pass per distinct key of a record
						// -- usually one or two. ----
						rep = false; best = rScore; uint32_t qw = lane;
						const unsigned long long recMask = ((2ull << (lastK - startK)) - 1ull) << startK;
						bool un = valid;
						for (;;)
						{
							const unsigned long long unAll = WBALLOT(un);
							if (!unAll) break;
							if (lane == 0) PSTAT(10, 1)
							const unsigned long long mine = unAll & recMask;
							const uint32_t f = mine ? (uint32_t)__ffsll(mine) - 1u : lane;
							const uint32_t kLo = WSHFL(keyLo, f), kHi = WSHFL(keyHi, f);
							const bool match = un & (keyLo == kLo) & (keyHi == kHi);
							float bs = match ? rScore : -3.0e38f; uint32_t bi = lane;
#define KAMD_POS_SEG(N) { const float os = IRORF(N, bs); const uint32_t oi = IROR(N, bi); const bool take = (il >= N) & (lane >= startK + N) & (os >= bs); bs = take ? os : bs; bi = take ? oi : bi; }
							KAMD_POS_SEG(1) KAMD_POS_SEG(2) KAMD_POS_SEG(4) KAMD_POS_SEG(8)
#undef KAMD_POS_SEG
#define KAMD_POS_CARRY(ROW) { const float os = __uint_as_float(WREADLANE(__float_as_uint(bs), 16 * ROW - 1)); const uint32_t oi = WREADLANE(bi, 16 * ROW - 1); const bool take = (irow == ROW) & (startK < 16u * ROW) & (os >= bs); bs = take ? os : bs; bi = take ? oi : bi; }
							KAMD_POS_CARRY(1) KAMD_POS_CARRY(2) KAMD_POS_CARRY(3)
#undef KAMD_POS_CARRY
							const float rb = WSHFL(bs, lastK); const uint32_t rq = WSHFL(bi, lastK);
							if (match && lane == f) { rep = true; best = rb; qw = rq; }
							un = un && !match;
						}
						PTL(5)
						wfcs = WSHFL(rFcs, qw);
						wtyp = WSHFL(rTypo, qw);
#ifdef KAMD_CONG
						wx1 = WSHFL(ctx, qw); wx2 = 0;
#else
						wx1 = nch1; wx2 = nch2;      // (the winner has this item's key, hence its LM node)
#endif
						wl = qw - startK; wNodeU = (uint32_t)lmNode; wHi = keyHi;
						wpar = WSHFL(pidx, qw);      // (the winner's parent state)
					}
					// ---- kept states stream to their group's arena, in item order ----
					uint32_t myRank = 0, myAdd = 0, ownerAdd = 0;
					for (uint32_t g2i = 0; g2i < NG; ++g2i)
					{
						const unsigned long long bg = WBALLOT(rep && owner == g2i);
						if (owner == g2i) { myRank = (uint32_t)__popcll(bg & lowerMask64); ownerAdd = (uint32_t)__popcll(bg); }
						if (grp == g2i) myAdd = (uint32_t)__popcll(bg);
					}
					if (rep) PSTAT(11, 1)
					if (rep)
					{
						const uint32_t pos = stTopO + myRank;
						// (the winner is an item of the same record: same candidate, same node, same key.  The LDS ring keeps the LAST PHR states: of more
						// than PHR states written in one round only those go into it, so that two lanes never write one slot)
						if (pos < stCapO && pos - posStartO < PST_CAP) emitState(pos, pos + PHR >= stTopO + ownerAdd, (int32_t)wNodeU, (uint8_t)wHi, (uint8_t)(wHi >> 8), best, wfcs, wtyp, wx1, wx2, wl, wpar);
						else ldsPtr<uint32_t>(ldsO + PosLay::OVFL)[0] = 1;
					}
					stTop += myAdd;
					ringTop = stTop > ringTop ? stTop : ringTop;
					if (gl == 0 && myAdd) { gctx[9] = stTop; gctx[11] = ringTop; }
					PTL(6)
					__syncthreads();
				}
			}
			}      // (passes)

			// ================= the groups again: pruning, retries, reachable flags, commit =================
			if (active && *ovfL) { stopAt = i0 | (5u << 24); active = false; }      // arena or staging full: the general kernel redoes the position (and reports a real overflow)
			if (active)
			{
				// ---- pruning (PathEvaluator.hpp:475-511): a path dies iff a socket-free path of its node and root lies more than cutOff above it; then every
				// new state adds itself to its node's counters (one LDS atomic: states | own-candidate states | live | live socket-free) ----
				const uint32_t cnt = stTop - posStart;
				if (gl == 0) PHIST(2, cnt)
				PTL(7)
				PBEACON(9, pi, cnt, attempt)
				// The best socket-free score per node of the position's COMMON-root states comes from one LDS float maximum per state (the reference's
				// bestPathValues, PathEvaluator.hpp:478-486) -- almost every state has the common root (others exist behind quotes / bullets only), and a state
				// of another root finds the best of its (node, root) by scanning the staged list.  (Rounds 3 / 4: fifteen row rotations per step.)
				LDS_AS float* pbest = ldsPtr<float>(lds + PosLay::PBEST);
				pbest[gl] = -INFINITY;
				waveSyncLds();
				bool otherRoot = false;
				for (uint32_t b = 0; b < cnt; b += G)
				{
					const uint32_t i = b + gl;
					if (i >= cnt) continue;
					const uint32_t bits = stB[i];
					if (bits & 0x1Fu) otherRoot = true;
					else if (!(bits & SB_MORPH_SOCKET)) ldsMaxF(&pbest[(bits >> 8) & 0xFu], stSc[i]);
				}
				waveSyncLds();
				const bool scanRoots = GBALLOT(otherRoot) != 0;
				for (uint32_t b = 0; b < cnt; b += G)
				{
					const uint32_t i = b + gl;
					if (i >= cnt) continue;
					const uint32_t bits = stB[i]; const float lim = stSc[i] + P.cutOff;
					bool kill = lim < pbest[(bits >> 8) & 0xFu];      // (a negative cutOff: the best path itself lies "above" itself)
					if (scanRoots && (bits & 0x1Fu))
					{
						kill = false;
						for (uint32_t j = 0; j < cnt; ++j)
						{
							const uint32_t bj = stB[j];
							if (!(bj & SB_MORPH_SOCKET) && (bj & 0xF1Fu) == (bits & 0xF1Fu) && lim < stSc[j]) kill = true;
						}
					}
					// (the ring copy only if the slot is still this state's: a step may write more than PHR states)
					if constexpr (kLiveOnly)
					{
						LDS_AS uint32_t* dwp = ldsPtr<uint32_t>(lds + PosLay::DWIN) + (((posStart + i) >> 5) & (PosLay::DWIN_WORDS - 1u));
						if (kill) ldsOr(dwp, 1u << ((posStart + i) & 31u)); else ldsAnd(dwp, ~(1u << ((posStart + i) & 31u)));
					}
					if (kill) { stArena()[posStart + i].dead = 1; if (ringTop - (posStart + i) <= PHR) ldsPtr<uint32_t>(hotR + 16 * ((posStart + i) & (PHR - 1)) + 12)[0] |= 1u << 16; }
					ldsAdd(&nCnt[(bits >> 8) & 0xFu], 1u | ((bits & PSB_PASS1) ? 0u : 1u << 8) | (kill ? 0u : 1u << 16) | ((kill || (bits & SB_STATE_SOCKET)) ? 0u : 1u << 24));
				}
				waveSyncLds();
				PTL(8)
				const uint32_t myC = nCnt[gl];      // of node i0 + gl
				const uint32_t myCnt = myC & 0xFFu, myP0 = (myC >> 8) & 0xFFu, myLive = (myC >> 16) & 0xFFu, myFree = myC >> 24;
				const bool isNode = gl < m, formNode = isNode && !((dq.z >> (16 + gl)) & 1u);      // (a formless node has no second reading, no fallback and no disconnection test)
				// ---- retries ----
				bool redo = false;
				if (attempt == 0)
				{
					const uint32_t lacking = GBALLOT(isNode && !myP0);
					if (lacking) { retry0 = lacking; attempt = 1; redo = true; }
				}
				if (!redo && attempt <= 1)
				{
					const uint32_t stateless = GBALLOT(isNode && !myCnt && ((dq.w >> gl) & 1u));
					if (stateless) { retry0 |= stateless; retry1 = stateless; attempt = 2; redo = true; }
				}
				if (redo && gl == 0) PSTAT(13, 1)
				if (redo) stTop = posStart;
				else
				{
				// ---- reachable flags; a dictionary node without a socket-free live path triggers the disconnected-lattice test (PathEvaluator.hpp:1286-1299):
				// its own flag is cleared, the flags of all later nodes are recomputed by propagation, and only if the end node comes out unreachable does the
				// node get the unknown-word fallback -- that (rare) evaluation is the general kernel's ----
				const uint32_t spJ = ppA >> 24;      // position my node's predecessors end at
				const uint32_t nonFree = GBALLOT(formNode && !myFree);
				if (gl == 0 && nonFree) { PSTAT(17, 1) if (!scanned) PSTAT(18, 1) }      // (developer statistics: steps that run the disconnected-lattice test / chunks that do so at least once)
				uint32_t flagBits = 0;      // bit j: flag of node i0 + j after its evaluation
				if (!nonFree) flagBits = GBALLOT(isNode && (formNode || tbit(aLast, spJ)));
				else
				{
					if (!canPropagate) { stopAt = i0 | (9u << 24); active = false; }      // (developer statistics: 9 = the test cannot run here -- a position with more than four start positions, or more than 255 positions --, 7 = it ran and the lattice is disconnected)
					else
					{
					const bool predFlag = isNode && tbit(aCur, spJ);
					flagBits = 0; bool disconnected = false;
					for (uint32_t j = 0; j < m; ++j)
					{
						const uint32_t spj = GSHFL(spJ, j);
						if (!((nonFree >> j) & 1u))
						{
							if (!((dq.z >> (16 + j)) & 1u) || tbit(aLast, spj)) flagBits |= 1u << j;
							continue;
						}
						// the test at node j: earlier siblings with their flags, later ones (not evaluated yet in the reference's order) by their predecessors'
						const uint32_t later = GBALLOT(predFlag && gl > j);
						if (gl < 8) aTmp[gl] = aCur[gl];
						waveSyncLds();
						if (flagBits || later) sbit(aTmp, pi);
						for (uint32_t x = pi + 1; x <= nPos; x += G)
						{
							uint32_t st4 = 0; TYPO_ONLY(uint32_t st8 = 0;)
							if (x + gl <= nPos) { st4 = posStarts(x + gl); TYPO_ONLY(st8 = W.posMask[nBase2 + x + gl];) }
							const uint32_t nx = nPos - x + 1 < (uint32_t)G ? nPos - x + 1 : (uint32_t)G;
							for (uint32_t t = 0; t < nx; ++t)
							{
								const uint32_t s4 = GSHFL(st4, t);
								uint32_t reached = tbit(aTmp, s4 & 0xFFu) | tbit(aTmp, (s4 >> 8) & 0xFFu) | tbit(aTmp, (s4 >> 16) & 0xFFu) | tbit(aTmp, s4 >> 24);
								TYPO_ONLY({ const uint32_t s8 = GSHFL(st8, t); reached |= tbit(aTmp, s8 & 0xFFu) | tbit(aTmp, (s8 >> 8) & 0xFFu) | tbit(aTmp, (s8 >> 16) & 0xFFu) | tbit(aTmp, s8 >> 24); })
								if (reached) sbit(aTmp, x + t);
							}
						}
						if (!tbit(aTmp, eosStart)) { disconnected = true; break; }
						waveSyncLds();
						if (gl < 8) aLast[gl] = aTmp[gl];
						waveSyncLds();
						scanned = true;
					}
					if (disconnected) { stopAt = i0 | (7u << 24); active = false; }
					}
				}

				if (active)
				{
				if (flagBits) sbit(aCur, pi);
				// ---- commit: state ranges of the nodes (ring + HBM tables), reachable flags ----
				PTL(9)
				PBEACON(10, pi, cnt, 0)
				const uint32_t inclBoth = grpScan<G>(isNode ? (myCnt | (myLive << 16)) : 0u, gl);      // (states and live states of the nodes so far: neither passes 16 bits)
				const uint32_t inclCnt = inclBoth & 0xFFFFu, inclLive = inclBoth >> 16;
				if (isNode)
				{
					const uint32_t i = i0 + gl, ns = posStart + inclCnt - myCnt;
					rBeg[i & (RING - 1)] = ns; rEnd[i & (RING - 1)] = ns + myCnt; rCum[i & (RING - 1)] = cumLive + inclLive;
					nodeStOff(i) = ns; nodeStCnt(i) = myCnt; nodeLive(i) = (uint16_t)myLive;
#ifdef KAMD_POS_TRACE
					fprintf(stderr, "commit pi %u node %u ns %u cnt %u live %u free %u p0 %u attempt %u\n", pi, i, ns, myCnt, myLive, myFree, myP0, attempt);
#endif
					reach(i) = (uint8_t)((flagBits >> gl) & 1u);      // (a formless node's flag is never set by its own evaluation: it keeps what the last test left, PathEvaluator.hpp:1300-1318)
				}
				cumLive += GSHFL(inclLive, G - 1);
				// next step: B becomes A
				dqA = dqB; dqB = dqC; ppA = ppB; rqA = rqB; recA0 = recB0; recA1 = recB1; recA2 = recB2;
				++pi; attempt = 0; retry0 = 0; retry1 = 0;
				waveSyncLds();
				PTL(10)
				if (pi > nPos)
				{
					// ---- end node, first half (PathEvaluator.hpp:1320-1358): the end-of-sentence transition of every path that may end the sentence -> the
			// end-candidate list k_finish_paths sorts and selects from, left in the unused tail of the chunk's state arena (what finishChunk does for
			// the general kernel: written out here once more so that this kernel holds no function call) ----
			{
				const uint32_t chunkE = gctx[12], Gn = gctx[15];
				const uint4 enq = reinterpret_cast<const uint4*>(&W.nodes[nBase + Gn - 1])[0];      // {form, start | end << 16, prev | sibling << 16, ...}
				const uint32_t enPrev = enq.z & 0xFFFFu, enNPrev = W.nodes[nBase + Gn - 1].nPrev;
				const uint32_t firstPrev = Gn - 1 - enPrev;
				const uint32_t pBegE = nodeStOff(firstPrev);
				const uint32_t nPE = (enPrev && enNPrev) ? nodeStOff(firstPrev + enNPrev - 1) + nodeStCnt(firstPrev + enNPrev - 1) - pBegE : 0u;
				DevState* st = stArena(); const uint8_t* uniq = uniqStates();
				EndCand* endBuf = reinterpret_cast<EndCand*>(st + stTop);
				const uint64_t freeBytes = (uint64_t)(stCap - stTop) * sizeof(DevState);
				const uint32_t endCap = freeBytes > (uint64_t)Gn * 4 ? (uint32_t)((freeBytes - (uint64_t)Gn * 4) / sizeof(EndCand)) : 0u;
				const bool openEnding = (B.chunkFlags[chunkE] & 1) != 0;
				const uint32_t nUniq = B.spOff[chunkE + 1] - B.spOff[chunkE];
				uint32_t nEnd = 0; bool endOverflow = false;
				for (uint32_t pb = 0; pb < nPE; pb += G)
				{
					const uint32_t p = pb + gl;
					bool ok = false; float c = 0, first = 0, ptypo = 0; uint8_t pRoot = 0, pSp = 0;
					if (p < nPE)
					{
						const uint4* ps4 = reinterpret_cast<const uint4*>(st + pBegE + p);
						const uint4 a = ps4[0], b2 = ps4[1];
						const MorphRec pm = M.morphs[b2.w];
						const uint8_t pSocket = (uint8_t)a.w, pDead = (uint8_t)(a.w >> 16);
						pRoot = (uint8_t)(a.z >> 16); pSp = (uint8_t)(a.z >> 24); ptypo = __uint_as_float(b2.x);
						ok = !pSocket && !pDead;
						if (ok && !(pm.flags & MF_SINGLE) && pm.nChunks <= (pm.socket ? 2u : 1u) && pm.vowel != CV_NONE) ok = false;   // isMatched(nullptr, vowel)
						if (ok && pm.tag == T_Z_SIOT) ok = false;
						if (ok)
						{
							c = __uint_as_float(a.y);
							if (!openEnding)
							{
								int32_t ln = (int32_t)a.x;
#ifdef KAMD_CONG
								uint32_t ectx = ps4[2].z;
								first = congStep(M, CGv, ln, ectx, 1u, false);
#else
								first = lmProgress(M, ln, 1);
#endif
								c += first;
								if (pSp & 1) c -= 2;
								if (pSp & 2) c -= 2;
							}
						}
					}
					const uint32_t mult = (ok && pRoot == COMMON_ROOT) ? nUniq : (ok ? 1u : 0u);
					const uint32_t incl = grpScan<G>(mult, gl);
					const uint32_t baseE = nEnd + incl - mult;
					for (uint32_t r = 0; r < mult; ++r)
					{
						if (baseE + r < endCap)
						{
							EndCand e; e.score = c; e.fcs = first; e.typo = ptypo; e.parent = pBegE + p; e.pad = 0;
							if (pRoot == COMMON_ROOT) { e.rootId = (uint8_t)r; e.sp = uniq[r]; } else { e.rootId = pRoot; e.sp = pSp; }
							endBuf[baseE + r] = e;
						}
						else endOverflow = true;
					}
					nEnd += GSHFL(incl, G - 1);
				}
				const bool anyOverflow = GBALLOT(endOverflow) != 0;
				if (gl == 0)
				{
					DevChunkResult* res = &W.results[chunkE];
					res->nEnd = nEnd; res->endOff = stTop; res->nPaths = 0;
					res->status = anyOverflow ? CS_ERR_STATE_OVERFLOW : CS_OK;
					res->pad = kPosChunkDone;
				}
			}
					active = false;
				}
				}
				}
			}
			__syncthreads();
		}

		const uint32_t chunkL = gctx[12], GnL = gctx[15];
		// handing over after a test: the flags it left for the nodes not evaluated yet go to the table the general kernel reads
		if (searching && stopAt && scanned)
			for (uint32_t k = (stopAt & 0xFFFFFFu) + gl; k + 1 < GnL; k += G) reach(k) = (uint8_t)tbit(aLast, posPrev(k) >> 24);
		PBEACON(11, stopAt, 0, 0)
#ifdef KAMD_POS_DEBUG
		PTL(11)
		if (W.beacon && mine && gl == 0) { volatile uint32_t* bq_ = W.beacon + 64ull * chunk; for (int k_ = 0; k_ < 14; ++k_) bq_[16 + k_] = tlAcc[k_]; bq_[31] = nPos; }
#endif
		// ---- A chunk the position steps could not finish (a lattice that really is disconnected, a record set they do not do, a full arena) goes on in
		// the general search at that node: same arena, same per-node tables.  The first W.posContSlots of them do so HERE, in this wavefront, while the
		// rest of the launch is still stepping (the longest chunks are dispatched first, so such a chunk's remaining chain -- about a millisecond for a
		// long sentence -- runs beside the other blocks instead of after them); any further ones are left to k_best_path, launched after this kernel. ----
		const bool handOver = searching && stopAt != 0;
		bool cont = false;
		uint32_t slot = 0xFFFFFFFFu;
		if (W.posScratch)
		{
			if (handOver) { if (gl == 0) slot = atomicAdd(W.posContCounter, 1u); slot = GSHFL(slot, 0); }
			cont = handOver && slot < W.posContSlots;
		}
		if constexpr (G == 8)
		{
			// The general search works in 16-lane groups: the (up to eight) chunks this wavefront carries on are listed in LDS and searched four at a time,
			// each by one 16-lane row of the wavefront -- every lane is free now, the steps of all eight groups have ended.
			const unsigned long long cm = WBALLOT(cont && gl == 0);
			if (cm)
			{
				__syncthreads();
				LDS_AS uint32_t* lst = ldsPtr<uint32_t>(PosLay::ROWMAP);      // (behind the general search's own layout: Lay<16>::TOTAL <= ROWMAP is asserted below)
				static_assert(Lay<16>::TOTAL <= PosLayT<8>::ROWMAP && 3 * 4 * (64 / 8) <= 128, "list of the chunks carried on");
				if (cont && gl == 0) { const uint32_t at = (uint32_t)__popcll(cm & lowerMask64); lst[3 * at] = chunkL; lst[3 * at + 1] = stopAt; lst[3 * at + 2] = slot; }
				const uint32_t nH = (uint32_t)__popcll(cm);
				LDS_AS float* lb = ldsPtr<float>(Lay<16>::LB);
				for (uint32_t t = lane; t < 2 * T_MAX + 1; t += 64)
				{
					float v = 0;
					if (t == 2 * T_MAX) v = 5.f;
					else if (t < T_MAX) { if (t == T_NNP || t == T_NP || t == T_IC) v = -1; else if (t == T_SB) v = -3; }
					else { const uint8_t r = (uint8_t)(t - T_MAX); v = (isEClass(r) || isJClass(r) || isSuffixTag(r) || r == T_VCP) ? -1.f : 0.f; }
					lb[t] = v;
				}
				__syncthreads();
#ifdef KAMD_HIPEMU
				hipemu_set_width(16);
#endif
				for (uint32_t base = 0; base < nH; base += 4)
				{
					const uint32_t e = base + irow;
					if (e < nH)
					{
						const uint32_t chunkE = lst[3 * e], stopE = lst[3 * e + 1], slotE = lst[3 * e + 2];
#ifdef KAMD_HIPEMU
						const PosKernArgs A{ M, B, W, P, chunkOrder, nWork TYPO_ONLY(, nodeTypoAll) CONG_ONLY(, CGv) };
						continueChunk(&A, chunkE, il, irow, slotE, stopE, W.posScratch, chunkOrder, nWork);
#else
						continueChunk(chunkE, il, irow, slotE, stopE, W.posScratch, chunkOrder, nWork);
#endif
					}
				}
#ifdef KAMD_HIPEMU
				hipemu_set_width(8);
#endif
			}
			if (handOver && !cont && gl == 0) { W.results[chunkL].pad = stopAt; *W.posHandOver = 1; }
		}
		else
		{
		if (handOver && !cont && gl == 0) { W.results[chunkL].pad = stopAt; *W.posHandOver = 1; }
		if (WBALLOT(cont))
		{
			__syncthreads();
			// the general search's LDS layout over this block's: per-group regions, then the left-boundary tag scores (k_best_path's prologue)
			LDS_AS float* lb = ldsPtr<float>(Lay<16>::LB);
			for (uint32_t t = lane; t < 2 * T_MAX + 1; t += 64)
			{
				float v = 0;
				if (t == 2 * T_MAX) v = 5.f;
				else if (t < T_MAX) { if (t == T_NNP || t == T_NP || t == T_IC) v = -1; else if (t == T_SB) v = -3; }
				else { const uint8_t r = (uint8_t)(t - T_MAX); v = (isEClass(r) || isJClass(r) || isSuffixTag(r) || r == T_VCP) ? -1.f : 0.f; }
				lb[t] = v;
			}
			__syncthreads();
			if (cont)
			{
#ifdef KAMD_HIPEMU
				const PosKernArgs A{ M, B, W, P, chunkOrder, nWork TYPO_ONLY(, nodeTypoAll) CONG_ONLY(, CGv) };
				continueChunk(&A, chunkL, gl, grp, slot, stopAt, W.posScratch, chunkOrder, nWork);
#else
				continueChunk(chunkL, gl, grp, slot, stopAt, W.posScratch, chunkOrder, nWork);
#endif
			}
		}
		}
#undef POS_LOADS_ARRIVED
#undef GBALLOT
#undef GSHFL
#undef WBALLOT
#undef WSHFL
#undef WREADLANE
#undef IROR
#undef IRORF
#undef PBEACON
#undef PTL
#undef PSTAT
#undef PHIST
	}
#endif
