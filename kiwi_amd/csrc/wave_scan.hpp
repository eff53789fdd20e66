// Wave-wide inclusive scans of a 64-lane wavefront (gfx950) on the DPP data path: no LDS crossbar (ds_bpermute), no lgkmcnt wait.
//
// EVERY helper here must be called with all 64 lanes of the wavefront active (uniform control flow): a DPP read from an inactive lane
// returns the `old` operand and v_readlane reads whatever the register of an inactive lane holds.
//
//   waveInclSum(x)                  x[0] + ... + x[lane]
//   waveSegInclSum(x, start)        x[max(start, first lane of the segment)] + ... + x[lane]
//   waveSegInclOr(lo, hi, start)    the same with OR over a 64-bit value held as two words (in place)
//   waveLast(x)                     the value of lane 63 (after an inclusive sum: the total)
//
// A segment is given per lane by `start`, the first lane of the segment the lane belongs to (start <= lane, equal for all lanes of a
// segment; 0 for a segment that began before lane 0).  Four Hillis-Steele steps inside every row of 16 lanes (row_shr:1/2/4/8: a source
// outside the row reads as 0), then the running value of the last lane of rows 0, 1 and 2 is carried into the next row, one row after
// the other, through an SGPR (v_readlane) -- a lane takes the carry when its segment began before its row.
// The lane emulator (KAMD_HIPEMU) implements row rotations only: there the helpers are the six-step __shfl_up loops.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace kamd
{
#ifdef KAMD_HIPEMU
	__device__ __forceinline__ uint32_t waveLast(uint32_t x) { return __shfl(x, 63); }
	__device__ __forceinline__ uint32_t waveInclSum(uint32_t x)
	{
		const uint32_t lane = threadIdx.x & 63u;
		for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(x, d); if (lane >= d) x += v; }
		return x;
	}
	__device__ __forceinline__ uint32_t waveSegInclSum(uint32_t x, uint32_t start)
	{
		const uint32_t lane = threadIdx.x & 63u;
		for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(x, d); if (lane >= d && lane - d >= start) x += v; }
		return x;
	}
	__device__ __forceinline__ void waveSegInclOr(uint32_t& lo, uint32_t& hi, uint32_t start)
	{
		const uint32_t lane = threadIdx.x & 63u;
		for (uint32_t d = 1; d < 64; d <<= 1)
		{
			const uint32_t vl = __shfl_up(lo, d), vh = __shfl_up(hi, d);
			if (lane >= d && lane - d >= start) { lo |= vl; hi |= vh; }
		}
	}
#else
	namespace wsdetail
	{
		// row_shr:D with old = 0 and bound_ctrl off: lane i of a row reads lane i - D of the same row, 0 when there is none
		template<int D> __device__ __forceinline__ uint32_t rowShr(uint32_t x) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x110 + D, 0xF, 0xF, false); }
		__device__ __forceinline__ uint32_t rowEnd(uint32_t x, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)x, lane); }
	}
	__device__ __forceinline__ uint32_t waveLast(uint32_t x) { return wsdetail::rowEnd(x, 63); }
	__device__ __forceinline__ uint32_t waveInclSum(uint32_t x)
	{
		using namespace wsdetail;
		const uint32_t lane = threadIdx.x & 63u;
		x += rowShr<1>(x); x += rowShr<2>(x); x += rowShr<4>(x); x += rowShr<8>(x);
		// (one row after the other: the carry out of a row includes what that row took from the row before)
		x += (lane >= 16 && lane < 32) ? rowEnd(x, 15) : 0u;
		x += (lane >= 32 && lane < 48) ? rowEnd(x, 31) : 0u;
		x += lane >= 48 ? rowEnd(x, 47) : 0u;
		return x;
	}
	__device__ __forceinline__ uint32_t waveSegInclSum(uint32_t x, uint32_t start)
	{
		using namespace wsdetail;
		const uint32_t lane = threadIdx.x & 63u;
		const uint32_t room = lane - start;      // how many lanes below this one belong to its segment
		uint32_t v;
		v = rowShr<1>(x); x += room >= 1 ? v : 0u;
		v = rowShr<2>(x); x += room >= 2 ? v : 0u;
		v = rowShr<4>(x); x += room >= 4 ? v : 0u;
		v = rowShr<8>(x); x += room >= 8 ? v : 0u;
		x += (lane >= 16 && lane < 32 && start < 16) ? rowEnd(x, 15) : 0u;
		x += (lane >= 32 && lane < 48 && start < 32) ? rowEnd(x, 31) : 0u;
		x += (lane >= 48 && start < 48) ? rowEnd(x, 47) : 0u;
		return x;
	}
	__device__ __forceinline__ void waveSegInclOr(uint32_t& lo, uint32_t& hi, uint32_t start)
	{
		using namespace wsdetail;
		const uint32_t lane = threadIdx.x & 63u;
		const uint32_t room = lane - start;
		uint32_t vl, vh;
		vl = rowShr<1>(lo); vh = rowShr<1>(hi); if (room >= 1) { lo |= vl; hi |= vh; }
		vl = rowShr<2>(lo); vh = rowShr<2>(hi); if (room >= 2) { lo |= vl; hi |= vh; }
		vl = rowShr<4>(lo); vh = rowShr<4>(hi); if (room >= 4) { lo |= vl; hi |= vh; }
		vl = rowShr<8>(lo); vh = rowShr<8>(hi); if (room >= 8) { lo |= vl; hi |= vh; }
		uint32_t cl, ch;
		cl = rowEnd(lo, 15); ch = rowEnd(hi, 15); if (lane >= 16 && lane < 32 && start < 16) { lo |= cl; hi |= ch; }
		cl = rowEnd(lo, 31); ch = rowEnd(hi, 31); if (lane >= 32 && lane < 48 && start < 32) { lo |= cl; hi |= ch; }
		cl = rowEnd(lo, 47); ch = rowEnd(hi, 47); if (lane >= 48 && start < 48) { lo |= cl; hi |= ch; }
	}
#endif
}
