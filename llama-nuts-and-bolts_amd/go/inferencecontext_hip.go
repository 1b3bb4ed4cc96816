//go:build hip

// inferencecontext_hip.go -- package model's InferenceContext on the MI355X library, selected with `-tags hip` (see
// llamatransformer_hip.go for how the two files slot under the reference's types).  Same exported names as
// src/model/inferencecontext.go:8-52: SequenceLength, CacheK, CacheV, NewInferenceContext(model, inferenceArgs, logFn), Logf.
//
// The KV cache lives on the device.  CacheK / CacheV are HOST MIRRORS with the reference's shape [SequenceLength, N_KVHeads, HeadDim]
// DT_BF16, allocated zero-filled like the reference (inferencecontext.go:32-42) and refreshed from the device by
// SyncCachesFromDevice -- after every Forward when MirrorCaches is set (what a test that reads CacheK, as
// llamatransformer_simulated_test.go:534-538 does, switches on), never otherwise (the copy is 2 x 64 KiB per token and layer).
//
// NOT COMPILED IN THIS REPOSITORY'S CI (no Go toolchain in the build image).

package model

/*
#include <stdint.h>
#include <stdlib.h>
#include "lnb.h"
extern void lnbGoLayerCallback(int layer, int nLayers, double secs, void* user);
*/
import "C"

import (
	"fmt"
	"runtime"
	"runtime/cgo"
	"unsafe"

	"github.com/adalkiran/llama-nuts-and-bolts/src/common"
	"github.com/adalkiran/llama-nuts-and-bolts/src/ml"
)

type InferenceContext struct {
	SequenceLength int // context size used during inference

	CacheK []*ml.Tensor // host mirrors, see SyncCachesFromDevice
	CacheV []*ml.Tensor

	MirrorCaches bool // refresh CacheK / CacheV after every Forward

	logFn func(format string, v ...any)

	handle *C.lnb_ctx
	lt     *LlamaTransformer // keeps the transformer alive (and finalized after this context)
	topK   int               // SetTokenProbs

	longContext bool // NewLongInferenceContext: created by lnb_ctx_create_long
	maxRows     int  // ... with activation buffers of this many rows (0: SequenceLength)
}

// LayerProgress switches the per-layer "Transformer block layer %d / %d was run" message (llamatransformer.go:163) on or off for
// contexts that were given a logFn.  The hook makes the library synchronise its stream after every block (that is what it times), which
// costs a few percent of a decode step: a host that only wants the text can set this to false.
var LayerProgress = true

// NewInferenceContext: same signature and defaults as src/model/inferencecontext.go:17-46.  The device side is created on the first
// Forward (the reference's constructor has no error return, and the context does not know its transformer until then).
func NewInferenceContext(model *Model, inferenceArgs common.InferenceArgs, logFn func(format string, v ...any)) *InferenceContext {
	context := &InferenceContext{logFn: logFn}
	if inferenceArgs.SequenceLength > 0 {
		context.SequenceLength = inferenceArgs.SequenceLength
	} else {
		context.SequenceLength = model.ModelArgs.MaxSequenceLength
	}
	modelArgs := model.ModelArgs
	context.CacheK = make([]*ml.Tensor, modelArgs.N_Layers)
	context.CacheV = make([]*ml.Tensor, modelArgs.N_Layers)
	for layerIdx := 0; layerIdx < modelArgs.N_Layers; layerIdx++ {
		context.CacheK[layerIdx], _ = ml.Zeros([]int{context.SequenceLength, modelArgs.N_KVHeads, modelArgs.HeadDim}, ml.DT_BF16)
		context.CacheV[layerIdx], _ = ml.Zeros([]int{context.SequenceLength, modelArgs.N_KVHeads, modelArgs.HeadDim}, ml.DT_BF16)
	}
	common.GLogger.DebugPrintf("Inference Context created with SequenceLength: %d", context.SequenceLength)
	return context
}

// NewLongInferenceContext: a context of up to 131072 positions (LNB_MAX_SEQ_LEN; lnb_ctx_create_long) whose per-call activation buffers hold
// maxRows rows instead of SequenceLength (0: SequenceLength).  The transformer's RoPE table must have SequenceLength rows; a Forward of more
// than maxRows rows is refused, so a long prompt goes in as chunks.  NewInferenceContext keeps the library's ~23000-position capacity.
func NewLongInferenceContext(model *Model, inferenceArgs common.InferenceArgs, maxRows int, logFn func(format string, v ...any)) *InferenceContext {
	context := NewInferenceContext(model, inferenceArgs, logFn)
	context.longContext = true
	context.maxRows = maxRows
	return context
}

// MaxRows: the rows per call the device-side activation buffers hold (lnb_ctx_max_rows); 0 before the first Forward has attached the context.
func (ic *InferenceContext) MaxRows() (int, error) {
	if ic.handle == nil {
		return 0, nil
	}
	var n C.int
	if err := lnbCall(func() C.int { return C.lnb_ctx_max_rows(ic.handle, &n) }); err != nil {
		return 0, err
	}
	return int(n), nil
}

func (ic *InferenceContext) Logf(format string, v ...any) {
	if ic.logFn != nil {
		ic.logFn(format, v...)
	}
}

// The library's per-layer hook (lnb_ctx_set_layer_callback) lands here and becomes the reference's
// infContext.Logf("Transformer block layer %d / %d was run, took %.4f sec(s)", ...) of llamatransformer.go:163.
//
//export lnbGoLayerCallback
func lnbGoLayerCallback(layer C.int, nLayers C.int, secs C.double, user unsafe.Pointer) {
	ic := cgo.Handle(uintptr(user)).Value().(*InferenceContext)
	ic.Logf("Transformer block layer %d / %d was run, took %.4f sec(s)", int(layer), int(nLayers), float64(secs))
}

var queueWarned bool // (guarded by lt.mu's critical section order: a benign race at worst prints the line twice)

// RuntimeInfo reports what lnb_runtime_info says about the process: hardware queues the HIP runtime was told to use (and, with probe, how many
// streams really run concurrently), whether the library's default arrived before HIP initialised, device and clocks.
type RuntimeInfo struct {
	ABIVersion, Device, NumCUs                             int
	ShaderClockKHz, MemoryClockKHz, WallClockKHz           int
	HWQueuesEnv, HWQueuesExpected, HWQueuesMeasured        int
	HWQueuesSetByLibrary, HIPInitialisedBeforeLibraryLoad  bool
	DeviceName, Arch                                       string
}

func GetRuntimeInfo(device int, probeQueues bool) (RuntimeInfo, error) {
	var ri C.lnb_runtime_info_t
	probe := C.int(0)
	if probeQueues {
		probe = 1
	}
	if err := lnbCall(func() C.int { return C.lnb_runtime_info(C.int(device), probe, &ri) }); err != nil {
		return RuntimeInfo{}, err
	}
	return RuntimeInfo{ABIVersion: int(ri.abi_version), Device: int(ri.device), NumCUs: int(ri.n_cus),
		ShaderClockKHz: int(ri.shader_clock_khz), MemoryClockKHz: int(ri.memory_clock_khz), WallClockKHz: int(ri.wall_clock_khz),
		HWQueuesEnv: int(ri.hw_queues_env), HWQueuesExpected: int(ri.hw_queues_expected), HWQueuesMeasured: int(ri.hw_queues_measured),
		HWQueuesSetByLibrary: ri.hw_queues_set_by_library != 0, HIPInitialisedBeforeLibraryLoad: ri.hip_initialised_before_load != 0,
		DeviceName: C.GoString(&ri.device_name[0]), Arch: C.GoString(&ri.arch[0])}, nil
}

// attach creates the device-side context on the first Forward.
func (ic *InferenceContext) attach(lt *LlamaTransformer) error {
	if ic.handle != nil {
		return nil
	}
	create := func() C.int { return C.lnb_ctx_create(lt.handle, C.int(ic.SequenceLength), &ic.handle) }
	if ic.longContext {
		create = func() C.int { return C.lnb_ctx_create_long(lt.handle, C.int(ic.SequenceLength), C.int(ic.maxRows), &ic.handle) }
	}
	if err := lnbCall(create); err != nil {
		return err
	}
	lt.mu.Lock()
	lt.ctxs++
	nctx := lt.ctxs
	lt.mu.Unlock()
	ic.lt = lt
	// One InferenceContext per generation, one goroutine each (inference.go:163-174): every context owns a HIP stream, and streams that
	// share a hardware queue run one after the other.  Say so ONCE when more contexts are alive than the runtime has queues.
	if nctx > 1 {
		var ri C.lnb_runtime_info_t
		if C.lnb_runtime_info(0, 0, &ri) == 0 && nctx > int(ri.hw_queues_expected) && !queueWarned {
			queueWarned = true
			common.GLogger.ConsolePrintf("warning: %d inference contexts on %d hardware queues: their steps will serialise", nctx, int(ri.hw_queues_expected))
		}
	}
	// Nothing pins the Go object: the reference creates one context per generation and never closes it (inference.go:174), so the
	// finalizer is what returns the device KV cache.  (A cgo.Handle held for the life of the context would keep it reachable for ever.)
	runtime.SetFinalizer(ic, func(c *InferenceContext) { c.Close() })
	return nil
}

// installLayerHook points the library's per-layer callback at this context for the duration of ONE Forward call: the cgo.Handle that
// lets the C side find the Go object exists only while the call runs (the callback fires synchronously inside lnb_forward, on the
// calling thread), so it never keeps the context alive.  The returned function removes the hook and deletes the handle.
func (ic *InferenceContext) installLayerHook() (release func(), err error) {
	if ic.logFn == nil || !LayerProgress {
		return func() {}, nil
	}
	h := cgo.NewHandle(ic)
	if err := lnbCall(func() C.int {
		return C.lnb_ctx_set_layer_callback(ic.handle, C.lnb_layer_cb(C.lnbGoLayerCallback), unsafe.Pointer(uintptr(h)))
	}); err != nil {
		h.Delete()
		return nil, err
	}
	return func() {
		C.lnb_ctx_set_layer_callback(ic.handle, nil, nil)
		h.Delete()
	}, nil
}

// SyncCachesFromDevice copies every layer's K and V cache into the host mirrors, in the reference's [position, kv head, dim] order
// (the library stores K position-contiguous on the device and hands it back transposed: lnb_ctx_read_kv).
func (ic *InferenceContext) SyncCachesFromDevice() error {
	if ic.handle == nil {
		return nil
	}
	for layer := range ic.CacheK {
		for which, t := range []*ml.Tensor{ic.CacheK[layer], ic.CacheV[layer]} {
			if err := lnbCall(func() C.int {
				return C.lnb_ctx_read_kv(ic.handle, C.int(layer), C.int(which), (*C.uint16_t)(unsafe.Pointer(&t.RawData[0])))
			}); err != nil {
				return err
			}
		}
	}
	return nil
}

// SetStopTokenIds hands model.Vocabulary.StopTokenIds to the device (lnb_ctx_set_stop_ids): the greedy loop then ends ON THE DEVICE with the
// first stop token (which is emitted, as inference.go:233-252 does), however many steps were enqueued behind it.  Up to 8 ids.
func (ic *InferenceContext) SetStopTokenIds(lt *LlamaTransformer, ids []TokenId) error {
	if err := ic.attach(lt); err != nil {
		return err
	}
	var p *C.int32_t
	if len(ids) > 0 {
		p = (*C.int32_t)(unsafe.Pointer(&ids[0]))
	}
	return lnbCall(func() C.int { return C.lnb_ctx_set_stop_ids(ic.handle, p, C.int(len(ids))) })
}

// DecodeGreedyUntil is the decode half of generateTokensInternal (inference.go:194-252) as ONE call: starting from `token` at position
// startPos it runs up to maxSteps Forward(1 token)+Argmax steps on the device and returns the tokens generated -- maxSteps of them unless a
// stop id ended the run (finished == true; the stop token is the last one).  The host loop that feeds generatedTokensCh calls it in chunks
// of any size: the tokens do not depend on the chunking.
func (ic *InferenceContext) DecodeGreedyUntil(lt *LlamaTransformer, token TokenId, startPos int, maxSteps int) (tokens []TokenId, finished bool, err error) {
	if maxSteps <= 0 { // &out[0] of an empty slice panics before the library can refuse the call
		return nil, false, fmt.Errorf("n_steps must be positive")
	}
	if err = ic.attach(lt); err != nil {
		return nil, false, err
	}
	out := make([]TokenId, maxSteps)
	var n, fin C.int
	if err = lnbCall(func() C.int {
		return C.lnb_decode_greedy_until(ic.handle, C.int32_t(token), C.int(startPos), C.int(maxSteps), (*C.int32_t)(unsafe.Pointer(&out[0])), &n, &fin, nil)
	}); err != nil {
		return nil, false, err
	}
	return out[:int(n)], fin != 0, nil
}

// Sampler mirrors lnb_sampler (include/lnb.h): Temperature 0 = greedy, TopK 0 = off, TopP 1 = off.  The sampled token is a function of the
// step's logits row, these four numbers and the position alone.
type Sampler struct {
	Temperature float32
	TopK        int
	TopP        float32
	Seed        uint64
}

// DecodeSampleUntil is DecodeGreedyUntil with the sampler's token in place of the argmax: the same stop ids, finished flag and chunking
// independence; the tokens are those of the rule in include/lnb.h, bit for bit the CPU restatement's.
func (ic *InferenceContext) DecodeSampleUntil(lt *LlamaTransformer, s Sampler, token TokenId, startPos int, maxSteps int) (tokens []TokenId, finished bool, err error) {
	if maxSteps <= 0 { // &out[0] of an empty slice panics before the library can refuse the call
		return nil, false, fmt.Errorf("n_steps must be positive")
	}
	if err = ic.attach(lt); err != nil {
		return nil, false, err
	}
	out := make([]TokenId, maxSteps)
	var n, fin C.int
	cs := C.lnb_sampler{temperature: C.float(s.Temperature), top_p: C.float(s.TopP), top_k: C.int32_t(s.TopK), reserved: 0, seed: C.uint64_t(s.Seed)}
	if err = lnbCall(func() C.int {
		return C.lnb_decode_sample_until(ic.handle, &cs, C.int32_t(token), C.int(startPos), C.int(maxSteps), (*C.int32_t)(unsafe.Pointer(&out[0])), &n, &fin, nil)
	}); err != nil {
		return nil, false, err
	}
	return out[:int(n)], fin != 0, nil
}

// SpecStats mirrors lnb_spec_stats: passes, passes that verified a draft, draft tokens verified, draft tokens emitted.
type SpecStats struct{ Passes, VerifyPasses, Drafted, Accepted int64 }

// SetDraft gives DecodeSpeculativeUntil its n-gram drafts: up to maxDraft (0..LNB_MAX_DRAFT; 0 = off, the default) tokens per pass, looked
// up with n-grams of ngramMin..ngramMax tokens in the running text, then in corpus (copied to the device; may be empty).
func (ic *InferenceContext) SetDraft(lt *LlamaTransformer, maxDraft int, ngramMin int, ngramMax int, corpus []TokenId) error {
	if err := ic.attach(lt); err != nil {
		return err
	}
	var p *C.int32_t
	if len(corpus) > 0 {
		p = (*C.int32_t)(unsafe.Pointer(&corpus[0]))
	}
	return lnbCall(func() C.int { return C.lnb_ctx_set_draft(ic.handle, C.int(maxDraft), C.int(ngramMin), C.int(ngramMax), p, C.int(len(corpus))) })
}

// SetBatchedAttention picks the attention form of DecodeSpeculativeUntil's verify passes: past longThreshold positions (negative: keep;
// default: never, unless the context is beyond the one-workgroup kernels' reach) the long-context kernels.  forceZseq 1: every column
// walks the serial f64 sum.  The bits are the same either way.
func (ic *InferenceContext) SetBatchedAttention(lt *LlamaTransformer, longThreshold int, forceZseq int) error {
	if err := ic.attach(lt); err != nil {
		return err
	}
	return lnbCall(func() C.int { return C.lnb_ctx_set_batched_attention(ic.handle, C.int(longThreshold), C.int(forceZseq)) })
}

// SetRowsAttention picks which appends run the multi-row long-context attention (lnb_ctx_set_rows_attention): calls of 2..15 rows (any row
// count at head_dim 32) past longThreshold positions (negative: keep; default: what the row-per-workgroup kernel cannot stage).  flags bit 0:
// every row walks the serial f64 sum; bit 1: the verify passes of DecodeSpeculativeUntil run it wherever they would run the long form.
func (ic *InferenceContext) SetRowsAttention(lt *LlamaTransformer, longThreshold int, flags int) error {
	if err := ic.attach(lt); err != nil {
		return err
	}
	return lnbCall(func() C.int { return C.lnb_ctx_set_rows_attention(ic.handle, C.int(longThreshold), C.int(flags)) })
}

// ForkPrefix copies this context's KV rows [0, nPos) of every layer into up to 128 (LNB_MAX_FORK) other contexts of the same transformer in one
// kernel launch (lnb_ctx_fork): a system prompt is prefilled once and shared.  Nothing but cache rows moves; continue each destination at nPos
// (ForwardAppend, DecodeGreedyUntil, DecodeSpeculativeUntil with the prefix as its history, a batch).  Capacities may differ.
func (ic *InferenceContext) ForkPrefix(lt *LlamaTransformer, dsts []*InferenceContext, nPos int) error {
	if len(dsts) == 0 { // &hs[0] of an empty slice panics before the library can refuse the call
		return fmt.Errorf("ForkPrefix: no destination")
	}
	if err := ic.attach(lt); err != nil {
		return err
	}
	hs := make([]*C.lnb_ctx, len(dsts))
	for i, d := range dsts {
		if d == nil {
			return fmt.Errorf("ForkPrefix: destination %d is nil", i)
		}
		if err := d.attach(lt); err != nil {
			return err
		}
		hs[i] = d.handle
	}
	// (the handles are C memory: a Go slice of C pointers may be passed to C)
	return lnbCall(func() C.int { return C.lnb_ctx_fork(ic.handle, C.int(nPos), (**C.lnb_ctx)(unsafe.Pointer(&hs[0])), C.int(len(hs))) })
}

// ForwardAppendMany extends up to 128 contexts of one transformer in one call (lnb_forward_append_many): context s takes tokens[s] at startPos[s], the
// rows of all of them packed into batched passes of up to 128 rows over the weights.  Every context's KV rows and its last row's argmax (the result,
// one per context) are bit-identical to its own ForwardAppend.  The step after ForkPrefix: each user's own text behind the shared prompt.
func ForwardAppendMany(lt *LlamaTransformer, ctxs []*InferenceContext, tokens [][]int32, startPos []int) ([]int32, error) {
	if len(ctxs) == 0 || len(tokens) != len(ctxs) || len(startPos) != len(ctxs) {
		return nil, fmt.Errorf("ForwardAppendMany: %d contexts, %d token lists, %d start positions", len(ctxs), len(tokens), len(startPos))
	}
	hs := make([]*C.lnb_ctx, len(ctxs))
	nRows := make([]C.int32_t, len(ctxs))
	pos := make([]C.int32_t, len(ctxs))
	var flat []C.int32_t
	for i, c := range ctxs {
		if c == nil {
			return nil, fmt.Errorf("ForwardAppendMany: context %d is nil", i)
		}
		if len(tokens[i]) == 0 {
			return nil, fmt.Errorf("ForwardAppendMany: context %d has no tokens", i)
		}
		if err := c.attach(lt); err != nil {
			return nil, err
		}
		hs[i] = c.handle
		nRows[i] = C.int32_t(len(tokens[i]))
		pos[i] = C.int32_t(startPos[i])
		for _, t := range tokens[i] {
			flat = append(flat, C.int32_t(t))
		}
	}
	argmax := make([]int32, len(ctxs))
	err := lnbCall(func() C.int {
		return C.lnb_forward_append_many((**C.lnb_ctx)(unsafe.Pointer(&hs[0])), C.int(len(hs)), &flat[0], &nRows[0], &pos[0], nil, (*C.int32_t)(unsafe.Pointer(&argmax[0])))
	})
	if err != nil {
		return nil, err
	}
	return argmax, nil
}

// SpecManyInfo is lnb_spec_many_info: the passes of one DecodeSpeculativeMany call, those with any draft, the sum and the maximum of their widths,
// the passes that ran the long-context attention pair.
type SpecManyInfo struct{ Passes, VerifyPasses, Columns, MaxColumns, LongPasses int64 }

// DecodeSpeculativeMany decodes up to 128 contexts of one transformer together (lnb_decode_speculative_many): every context drafts for itself with its
// own SetDraft settings and ONE batched pass over the weights verifies all of them.  Context s continues from tokens[s] at startPos[s] (histories[s]:
// the tokens before it; startPos[s] < 0: skipped, as a finished member of a chunked run).  colBudget: columns per pass, 0 = 16 * ceil(n / 16).  Every
// context's tokens, finished flag and KV cache rows are bit-identical to its own DecodeGreedyUntil.
func DecodeSpeculativeMany(lt *LlamaTransformer, ctxs []*InferenceContext, histories [][]TokenId, tokens []TokenId, startPos []int, maxSteps int, colBudget int) (out [][]TokenId, finished []bool, stats []SpecStats, info SpecManyInfo, err error) {
	return decodeSpeculativeMany(lt, ctxs, nil, histories, tokens, startPos, maxSteps, colBudget)
}

// DecodeSpeculativeSampleMany is DecodeSpeculativeMany with one sampler per context (lnb_decode_speculative_sample_many): every context's tokens,
// finished flag and KV cache rows are bit-identical to its own DecodeSampleUntil -- the sampler's draw depends on (seed, position) only, so the
// drafts are accepted by plain comparison and no rejection sampling is involved.  A Temperature-0 member is greedy.
func DecodeSpeculativeSampleMany(lt *LlamaTransformer, ctxs []*InferenceContext, samplers []Sampler, histories [][]TokenId, tokens []TokenId, startPos []int, maxSteps int, colBudget int) (out [][]TokenId, finished []bool, stats []SpecStats, info SpecManyInfo, err error) {
	if len(samplers) != len(ctxs) || len(samplers) == 0 {
		return nil, nil, nil, info, fmt.Errorf("DecodeSpeculativeSampleMany: %d samplers for %d contexts", len(samplers), len(ctxs))
	}
	return decodeSpeculativeMany(lt, ctxs, samplers, histories, tokens, startPos, maxSteps, colBudget)
}

// samplers nil: the greedy call
func decodeSpeculativeMany(lt *LlamaTransformer, ctxs []*InferenceContext, samplers []Sampler, histories [][]TokenId, tokens []TokenId, startPos []int, maxSteps int, colBudget int) (out [][]TokenId, finished []bool, stats []SpecStats, info SpecManyInfo, err error) {
	n := len(ctxs)
	if n == 0 || len(histories) != n || len(tokens) != n || len(startPos) != n {
		return nil, nil, nil, info, fmt.Errorf("DecodeSpeculativeMany: %d contexts, %d histories, %d tokens, %d start positions", n, len(histories), len(tokens), len(startPos))
	}
	if maxSteps <= 0 {
		return nil, nil, nil, info, fmt.Errorf("max_steps must be positive")
	}
	hs := make([]*C.lnb_ctx, n)
	hn := make([]C.int32_t, n)
	pos := make([]C.int32_t, n)
	tok := make([]C.int32_t, n)
	total := 0
	for i, c := range ctxs {
		if c == nil {
			return nil, nil, nil, info, fmt.Errorf("DecodeSpeculativeMany: context %d is nil", i)
		}
		if err = c.attach(lt); err != nil {
			return nil, nil, nil, info, err
		}
		hs[i], hn[i], pos[i], tok[i] = c.handle, C.int32_t(len(histories[i])), C.int32_t(startPos[i]), C.int32_t(tokens[i])
		total += len(histories[i])
	}
	// the histories and the array of pointers to them live in C memory: a Go slice of Go pointers must not be passed to C
	flat := (*C.int32_t)(C.malloc(C.size_t(4 * (total + 1))))
	hp := (**C.int32_t)(C.malloc(C.size_t(n) * C.size_t(unsafe.Sizeof(uintptr(0)))))
	defer C.free(unsafe.Pointer(flat))
	defer C.free(unsafe.Pointer(hp))
	flatS := unsafe.Slice(flat, total+1)
	hpS := unsafe.Slice(hp, n)
	at := 0
	for i, h := range histories {
		hpS[i] = nil
		if len(h) > 0 {
			hpS[i] = &flatS[at]
		}
		for _, t := range h {
			flatS[at] = C.int32_t(t)
			at++
		}
	}
	buf := make([]TokenId, n*maxSteps)
	ng := make([]C.int32_t, n)
	fin := make([]C.int32_t, n)
	st := make([]C.lnb_spec_stats, n)
	var ci C.lnb_spec_many_info
	cs := make([]C.lnb_sampler, len(samplers))
	for i, s := range samplers {
		cs[i] = C.lnb_sampler{temperature: C.float(s.Temperature), top_p: C.float(s.TopP), top_k: C.int32_t(s.TopK), reserved: 0, seed: C.uint64_t(s.Seed)}
	}
	if err = lnbCall(func() C.int {
		if samplers != nil {
			return C.lnb_decode_speculative_sample_many((**C.lnb_ctx)(unsafe.Pointer(&hs[0])), C.int(n), &cs[0], hp, &hn[0], &tok[0], &pos[0], C.int(maxSteps), C.int(colBudget),
				(*C.int32_t)(unsafe.Pointer(&buf[0])), &ng[0], &fin[0], &st[0], &ci, nil)
		}
		return C.lnb_decode_speculative_many((**C.lnb_ctx)(unsafe.Pointer(&hs[0])), C.int(n), hp, &hn[0], &tok[0], &pos[0], C.int(maxSteps), C.int(colBudget),
			(*C.int32_t)(unsafe.Pointer(&buf[0])), &ng[0], &fin[0], &st[0], &ci, nil)
	}); err != nil {
		return nil, nil, nil, info, err
	}
	for i := 0; i < n; i++ {
		out = append(out, buf[i*maxSteps:i*maxSteps+int(ng[i])])
		finished = append(finished, fin[i] != 0)
		stats = append(stats, SpecStats{int64(st[i].passes), int64(st[i].verify_passes), int64(st[i].drafted), int64(st[i].accepted)})
	}
	info = SpecManyInfo{int64(ci.passes), int64(ci.verify_passes), int64(ci.columns), int64(ci.max_columns), int64(ci.long_passes)}
	return out, finished, stats, info, nil
}

// SavePrefix returns the KV rows [0, nPos) as a capacity-independent blob (lnb_ctx_save_prefix; layout in lnb.h): a prefix cache in host memory
// or on disk.  The blob carries no model identity -- loading rows that other weights computed is the caller's mistake.
func (ic *InferenceContext) SavePrefix(lt *LlamaTransformer, nPos int) ([]byte, error) {
	if err := ic.attach(lt); err != nil {
		return nil, err
	}
	var n C.int64_t
	if err := lnbCall(func() C.int {
		n = C.lnb_ctx_prefix_bytes(ic.handle, C.int(nPos))
		if n < 0 {
			return -1
		}
		return 0
	}); err != nil {
		return nil, err
	}
	blob := make([]byte, int(n))
	if err := lnbCall(func() C.int { return C.lnb_ctx_save_prefix(ic.handle, C.int(nPos), unsafe.Pointer(&blob[0]), n) }); err != nil {
		return nil, err
	}
	return blob, nil
}

// LoadPrefix writes a saved prefix into rows [0, nPos) of this context and returns nPos (lnb_ctx_load_prefix); a blob of another geometry or
// stage range, a damaged one, or more positions than the context holds are refused before anything is written.
func (ic *InferenceContext) LoadPrefix(lt *LlamaTransformer, blob []byte) (int, error) {
	if len(blob) == 0 {
		return 0, fmt.Errorf("LoadPrefix: empty blob")
	}
	if err := ic.attach(lt); err != nil {
		return 0, err
	}
	var n C.int
	err := lnbCall(func() C.int { return C.lnb_ctx_load_prefix(ic.handle, unsafe.Pointer(&blob[0]), C.int64_t(len(blob)), &n) })
	return int(n), err
}

// AppendAttentionForm reports the attention of the last append: 0 none yet or one row, 1 the row-per-workgroup kernel, 2 the matrix-core
// kernel, 3 one-token steps inside the call, 4 the multi-row long-context pair.
func (ic *InferenceContext) AppendAttentionForm(lt *LlamaTransformer) (int, error) {
	if err := ic.attach(lt); err != nil {
		return 0, err
	}
	var f C.int
	err := lnbCall(func() C.int { return C.lnb_ctx_append_attention_form(ic.handle, &f) })
	return int(f), err
}

// VerifyAttentionForm reports what the last verify pass ran: 0 the one-workgroup attention kernels, 1 the long-context pair, 2 the multi-row pair.
func (ic *InferenceContext) VerifyAttentionForm(lt *LlamaTransformer) (int, error) {
	if err := ic.attach(lt); err != nil {
		return 0, err
	}
	var f C.int
	err := lnbCall(func() C.int { return C.lnb_ctx_verify_attention_form(ic.handle, &f) })
	return int(f), err
}

// DecodeSpeculativeUntil is DecodeGreedyUntil with drafts verified in batched passes over the weights: the same tokens, finished flag and
// KV cache rows, fewer passes when the text repeats itself or the corpus.  history: the tokens before `token` (the prompt).
func (ic *InferenceContext) DecodeSpeculativeUntil(lt *LlamaTransformer, history []TokenId, token TokenId, startPos int, maxSteps int) (tokens []TokenId, finished bool, stats SpecStats, err error) {
	return ic.decodeSpeculative(lt, nil, history, token, startPos, maxSteps)
}

// DecodeSpeculativeSampleUntil is DecodeSampleUntil with drafts verified in batched passes (lnb_decode_speculative_sample_until): the same tokens,
// finished flag and KV cache rows whatever the draft settings, because the sampler's draw depends on (seed, position) only.
func (ic *InferenceContext) DecodeSpeculativeSampleUntil(lt *LlamaTransformer, s Sampler, history []TokenId, token TokenId, startPos int, maxSteps int) (tokens []TokenId, finished bool, stats SpecStats, err error) {
	return ic.decodeSpeculative(lt, &s, history, token, startPos, maxSteps)
}

// s nil: the greedy loop
func (ic *InferenceContext) decodeSpeculative(lt *LlamaTransformer, s *Sampler, history []TokenId, token TokenId, startPos int, maxSteps int) (tokens []TokenId, finished bool, stats SpecStats, err error) {
	if maxSteps <= 0 {
		return nil, false, stats, fmt.Errorf("max_steps must be positive")
	}
	if err = ic.attach(lt); err != nil {
		return nil, false, stats, err
	}
	out := make([]TokenId, maxSteps)
	var h *C.int32_t
	if len(history) > 0 {
		h = (*C.int32_t)(unsafe.Pointer(&history[0]))
	}
	var n, fin C.int
	var st C.lnb_spec_stats
	if err = lnbCall(func() C.int {
		if s != nil {
			cs := C.lnb_sampler{temperature: C.float(s.Temperature), top_p: C.float(s.TopP), top_k: C.int32_t(s.TopK), reserved: 0, seed: C.uint64_t(s.Seed)}
			return C.lnb_decode_speculative_sample_until(ic.handle, &cs, h, C.int(len(history)), C.int32_t(token), C.int(startPos), C.int(maxSteps),
				(*C.int32_t)(unsafe.Pointer(&out[0])), &n, &fin, &st, nil)
		}
		return C.lnb_decode_speculative_until(ic.handle, h, C.int(len(history)), C.int32_t(token), C.int(startPos), C.int(maxSteps),
			(*C.int32_t)(unsafe.Pointer(&out[0])), &n, &fin, &st, nil)
	}); err != nil {
		return nil, false, stats, err
	}
	stats = SpecStats{int64(st.passes), int64(st.verify_passes), int64(st.drafted), int64(st.accepted)}
	return out[:int(n)], fin != 0, stats, nil
}

// SetTokenProbs makes the greedy loops record, for every token they generate, the topK (0..LNB_MAX_TOP_K; 0 = off, the default) most likely
// tokens of its logits row with their probabilities -- the bits of the reference's ml.Softmax on that row (include/lnb.h).
func (ic *InferenceContext) SetTokenProbs(lt *LlamaTransformer, topK int) error {
	if err := ic.attach(lt); err != nil {
		return err
	}
	if err := lnbCall(func() C.int { return C.lnb_ctx_set_token_probs(ic.handle, C.int(topK)) }); err != nil {
		return err
	}
	ic.topK = topK
	return nil
}

// TokenProbs returns records [first, first+n) of the last greedy call: ids, logits and probs [n*k] (entry i*k is the generated token) and
// ln Z [n] of each row.
func (ic *InferenceContext) TokenProbs(first int, n int) (ids []TokenId, logits []float32, probs []float32, logZ []float64, err error) {
	if ic.handle == nil {
		return nil, nil, nil, nil, fmt.Errorf("inference context is closed")
	}
	k := ic.topK
	ids, logits, probs, logZ = make([]TokenId, n*k+1), make([]float32, n*k+1), make([]float32, n*k+1), make([]float64, n+1)
	if err = lnbCall(func() C.int {
		return C.lnb_ctx_read_token_probs(ic.handle, C.int(first), C.int(n), (*C.int32_t)(unsafe.Pointer(&ids[0])), (*C.float)(unsafe.Pointer(&logits[0])),
			(*C.float)(unsafe.Pointer(&probs[0])), (*C.double)(unsafe.Pointer(&logZ[0])))
	}); err != nil {
		return nil, nil, nil, nil, err
	}
	return ids[:n*k], logits[:n*k], probs[:n*k], logZ[:n], nil
}

// Score runs Forward(tokens, startPos) and reports, per row, the logit and probability of targets[i] (a negative id: NaN) and ln Z,
// instead of the logits (lnb_forward_score); argmaxLast is Forward's next token.
func (ic *InferenceContext) Score(lt *LlamaTransformer, tokens []TokenId, startPos int, targets []TokenId) (targetLogit []float32, targetProb []float32, logZ []float64, argmaxLast TokenId, err error) {
	if len(tokens) == 0 || len(targets) != len(tokens) {
		return nil, nil, nil, -1, fmt.Errorf("Score: one target per token, at least one token")
	}
	if err = ic.attach(lt); err != nil {
		return nil, nil, nil, -1, err
	}
	n := len(tokens)
	targetLogit, targetProb, logZ = make([]float32, n), make([]float32, n), make([]float64, n)
	var am C.int32_t
	if err = lnbCall(func() C.int {
		return C.lnb_forward_score(ic.handle, (*C.int32_t)(unsafe.Pointer(&tokens[0])), C.int(n), C.int(startPos), (*C.int32_t)(unsafe.Pointer(&targets[0])),
			(*C.float)(unsafe.Pointer(&targetLogit[0])), (*C.float)(unsafe.Pointer(&targetProb[0])), (*C.double)(unsafe.Pointer(&logZ[0])), &am)
	}); err != nil {
		return nil, nil, nil, -1, err
	}
	return targetLogit, targetProb, logZ, TokenId(am), nil
}

// SetThroughputSchedule selects the co-residency-friendly forms of the one-token kernels (lnb_ctx_set_schedule): for hosts that keep several
// generations in flight on one GPU, one InferenceContext each (inference.go:174).  Same tokens either way.
func (ic *InferenceContext) SetThroughputSchedule(lt *LlamaTransformer, on bool) error {
	if err := ic.attach(lt); err != nil {
		return err
	}
	s := C.int(C.LNB_SCHED_LATENCY)
	if on {
		s = C.int(C.LNB_SCHED_THROUGHPUT)
	}
	return lnbCall(func() C.int { return C.lnb_ctx_set_schedule(ic.handle, s) })
}

// Close frees the device buffers of this context (idempotent; also run by the finalizer, before the transformer's).  The library refuses to
// destroy a context that a live batch still holds (its tables and captured graphs keep the device pointers): the handle is kept then.
func (ic *InferenceContext) Close() error {
	if ic.handle == nil {
		return nil
	}
	if err := lnbCall(func() C.int { return C.lnb_ctx_destroy(ic.handle) }); err != nil {
		return err
	}
	ic.handle = nil
	ic.lt.mu.Lock()
	ic.lt.ctxs--
	ic.lt.mu.Unlock()
	return nil
}
