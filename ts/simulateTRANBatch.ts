// ts/simulateTRANBatch.ts — many circuits' transients in as few launches as their topologies allow (spicey_amd/batch.py).
// Slot i is what simulateTRAN(ckts[i], options) returns, with the same state write-back; null for a circuit without .tran;
// an Error("Singular matrix (real)") object, returned instead of thrown, for a circuit whose run is singular (its state is
// left as it was).  Circuits that share node count, element order and nodes, recorded nodes, dt and step count run as the
// instances of one handle, each with its own source table.
import type { ParsedCircuit } from "./types"
import { computeEffectiveTimeStep, flatten } from "./simulateTRAN"
import { runTransientBatchNative, SPICEY_ERR_SINGULAR, type FlatCircuit, type NativeTranResult } from "./spiceyHip"

export type SimulateTranBatchOptions = {
  /** the reference's own algorithm (simulateTRAN's exactOrder): every slot bit-identical to a solo run */
  exactOrder?: boolean
  /** skipRisk (default true); false lets the handles take the throughput geometry, K = 4 and the hybrid kernel */
  diagnostics?: boolean
  /** instances per launch (default 4096): larger groups run as consecutive launches, which bounds the host buffers */
  maxInstances?: number
}

type Prepared = { ckt: ParsedCircuit; flat: FlatCircuit; recorded: number[]; dt: number; steps: number; src: Float64Array; times: number[]; key: string }

function prepare(ckt: ParsedCircuit): Prepared {
  const { dt: dtRequested, tstop } = ckt.analyses.tran!
  const { dt, steps } = computeEffectiveTimeStep(dtRequested, tstop)
  const nV = ckt.V.length
  const src = new Float64Array((steps + 1) * nV)
  const times: number[] = []
  let t = 0
  for (let step = 0; step <= steps; step++, t = step * dt) {
    times.push(t)
    for (let k = 0; k < nV; k++) {
      const vs = ckt.V[k]!
      src[step * nV + k] = vs.waveform ? vs.waveform(t) : vs.dc || 0
    }
  }
  const flat = flatten(ckt)
  const wanted = ckt.probes.tran.map((p) => p.toUpperCase())
  const recorded: number[] = []
  for (let id = 1; id <= flat.nNodes; id++) {
    if (wanted.length === 0 || wanted.includes(ckt.nodes.rev[id]!.toUpperCase())) recorded.push(id)
  }
  if (wanted.length > 0) flat.outNodes = Int32Array.from(recorded)
  const topo = [flat.R.n1, flat.R.n2, flat.C.n1, flat.C.n2, flat.L.n1, flat.L.n2, flat.V.n1, flat.V.n2, flat.S.n1, flat.S.n2, flat.S.cp, flat.S.cn, flat.D.np, flat.D.nm]
  const key = JSON.stringify([flat.nNodes, topo.map((a) => Array.from(a)), wanted.length > 0 ? recorded : null, dt, steps])
  return { ckt, flat, recorded, dt, steps, src, times, key }
}

/** simulateTRAN's re-keying and state write-back for one finished instance */
function finish(p: Prepared, res: NativeTranResult) {
  const { ckt, recorded, steps } = p
  const np1 = steps + 1
  const column = (buf: Float64Array, stride: number, col: number): number[] => {
    const out = new Float64Array(np1)
    for (let s = 0, k = col; s < np1; s++, k += stride) out[s] = buf[k]!
    return Array.from(out)
  }
  const nodeVoltages: Record<string, number[]> = {}
  recorded.forEach((id, c) => (nodeVoltages[ckt.nodes.rev[id]!] = column(res.outV, recorded.length, c)))
  const names = [
    ...ckt.R.map((e) => e.name), ...ckt.C.map((e) => e.name), ...ckt.L.map((e) => e.name), ...ckt.V.map((e) => e.name),
    ...ckt.S.filter((s) => s.model).map((e) => e.name), ...ckt.D.filter((d) => d.model).map((e) => e.name),
  ]
  const nCur = names.length
  const elementCurrents: Record<string, number[]> = {}
  const columnsOf: Map<string, number[]> = new Map()
  names.forEach((nm, j) => {
    const cols = columnsOf.get(nm)
    if (cols) cols.push(j)
    else columnsOf.set(nm, [j])
  })
  for (const [nm, cols] of columnsOf) {
    if (cols.length === 1) {
      elementCurrents[nm] = column(res.outI, nCur, cols[0]!)
    } else {
      const out: number[] = []
      for (let s = 0; s < np1; s++) for (const j of cols) out.push(res.outI[s * nCur + j]!)
      elementCurrents[nm] = out
    }
  }
  ckt.C.forEach((c, i) => (c.vPrev = res.state.vPrev[i]!))
  ckt.L.forEach((l, i) => (l.iPrev = res.state.iPrev[i]!))
  ckt.D.filter((d) => d.model).forEach((d, i) => (d.vdPrev = res.state.vdPrev[i]!))
  ckt.S.filter((s) => s.model).forEach((s, i) => (s.isOn = res.state.isOn[i] !== 0))
  return { times: p.times, nodeVoltages, elementCurrents, skipRisk: res.skipRisk }
}

export function simulateTRANBatch(ckts: ParsedCircuit[], options?: SimulateTranBatchOptions) {
  if (new Set(ckts).size !== ckts.length) throw new Error("simulateTRANBatch: the same circuit object appears twice")
  const maxInstances = options?.maxInstances ?? 4096
  if (!(maxInstances >= 1)) throw new Error("simulateTRANBatch: maxInstances must be >= 1")
  const out: (ReturnType<typeof finish> | null | Error)[] = ckts.map(() => null)
  const groups: Map<string, number[]> = new Map()
  const prepared: (Prepared | null)[] = ckts.map((c) => (c.analyses.tran ? prepare(c) : null))
  prepared.forEach((p, i) => {
    if (!p) return
    const g = groups.get(p.key)
    if (g) g.push(i)
    else groups.set(p.key, [i])
  })
  const native = { interpreter: options?.exactOrder ? 3 : 0, diagnostics: options?.diagnostics !== false }
  const launches: number[][] = []
  for (const g of groups.values()) for (let a = 0; a < g.length; a += maxInstances) launches.push(g.slice(a, a + maxInstances))
  for (const idx of launches) {
    let pending = idx
    while (pending.length) {
      if (pending !== idx) pending.forEach((i) => (prepared[i] = prepare(ckts[i]!)))  // (from the state the circuit still holds)
      const ps = pending.map((i) => prepared[i]!)
      const { steps, dt } = ps[0]!
      const shared = ps.every((p) => p.src.length === ps[0]!.src.length && p.src.every((v, k) => Object.is(v, ps[0]!.src[k])))
      let src = ps[0]!.src
      if (!shared) {
        src = new Float64Array(ps.length * ps[0]!.src.length)
        ps.forEach((p, j) => src.set(p.src, j * p.src.length))
      }
      const r = runTransientBatchNative(ps.map((p) => p.flat), steps, dt, src, !shared, native)
      const again: number[] = []
      pending.forEach((i, j) => {
        const s = r.status[j]!
        if (s === 0) {
          const res = finish(ps[j]!, r.results[j]!)
          out[i] = native.diagnostics ? res : { ...res, skipRisk: null as unknown as number }
        } else if (s === SPICEY_ERR_SINGULAR) out[i] = new Error("Singular matrix (real)")
        else if (s === -1) again.push(i)
        else throw new Error(`simulateTRANBatch: native error ${s}`)
      })
      if (again.length === pending.length) throw new Error("simulateTRANBatch: a launch settled none of its instances")
      pending = again
    }
  }
  return out
}
