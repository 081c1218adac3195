-- depth_estimation_api.lua -- the reference's public entry point, nextFrameDepth() (depth_estimation_api.lua:134-198: what
-- ardrone/ardrone_api.cpp:77-84 calls once per camera frame), over libdfe's stream object (include/dfe.h: dfe_stream_*).
-- UNTESTED here (no Lua runtime in the build image); the same entry points run under tests/ through the ctypes binding
-- (depth-estimation_amd/stream.py is this file's Python twin).
--   local api = require 'depth_estimation_api'
--   api.init{geometry = geometry, filter = loaded.filter, K = K, distP = distP, camera = cam}    -- what the script's top level sets up
--   function nextFrameDepth() return api.nextFrameDepth() end                                    -- im_scaled, xflow, mask
-- geometry: hImg, wImg, maxh, maxw, output_extraction_method ('max' / 'mean'; the script sets 'mean', :31); filter: getFilter's
-- nn.Sequential of nn.SpatialConvolution [+ nn.Tanh] (full connection), or nil for raw frames; K 3 x 3, distP 5 (nil: no undistortion);
-- camera: an object with :getNextFrame() -> FloatTensor C x H x W (ImageLoader / ImageCamera, :53-66).  Optional: rectify ('features' as
-- the script, or 'image' as test_opticalflow.lua:284), threshold, fix_mask_offset, min_inlier_ratio (0.2, :159), and the sfm table's
-- max_points, points_quality, points_min_dist, tracker_win_size, ransac2_max_dist (the .cal files' names).
local dfe = require 'dfe_ffi'
local ffi = require 'ffi'

local M = {}
local S = nil   -- the open stream: handle, params, device buffers, host tensors

-- the filter's parameters go to the device once; the stream copies the layer array and reads the weights from there on every push
local function filter_layers(filter, keep)
   if not filter then return nil, 0 end
   local layers, n = {}, 0
   for _, m in ipairs(filter.modules) do
      local tn = torch.typename(m)
      if tn == 'nn.Tanh' then
         if n == 0 then error('depth_estimation_api: the filter starts with nn.Tanh') end
         layers[n].tanh_after = 1
      elseif tn == 'nn.SpatialConvolution' then
         n = n + 1
         local bw, bb = dfe.newBuffer(), dfe.newBuffer()
         keep[#keep + 1] = bw; keep[#keep + 1] = bb
         layers[n] = {nIn = m.nInputPlane, nOut = m.nOutputPlane, kH = m.kH, kW = m.kW, tanh_after = 0,
                      weight = ffi.cast('const float*', (dfe.upload(m.weight, bw))), bias = ffi.cast('const float*', (dfe.upload(m.bias, bb)))}
      else
         error('depth_estimation_api: unsupported filter module ' .. tostring(tn))
      end
   end
   local arr = ffi.new('dfe_filter_layer[?]', n)
   for i = 1, n do
      local L, a = layers[i], arr[i - 1]
      a.nIn, a.nOut, a.kH, a.kW, a.weight, a.bias, a.conn, a.nConn, a.tanh_after = L.nIn, L.nOut, L.kH, L.kW, L.weight, L.bias, nil, 0, L.tanh_after
   end
   return arr, n
end

local function open(frame)
   local o = M.opt
   local g = o.geometry
   local p = ffi.new('dfe_stream_params')
   p.C, p.Hsrc, p.Wsrc, p.hImg, p.wImg = frame:size(1), frame:size(2), frame:size(3), g.hImg, g.wImg
   for i = 1, 3 do for j = 1, 3 do p.K[(i - 1) * 3 + j - 1] = o.K[i][j] end end
   p.has_dist = o.distP and 1 or 0
   if o.distP then for i = 1, 5 do p.dist[i - 1] = o.distP[i] end end
   local keep = {}
   local arr, n = filter_layers(o.filter, keep)
   p.layers, p.nlayers = arr, n
   p.maxh, p.maxw = g.maxh, g.maxw
   p.extraction = (g.output_extraction_method == 'mean') and 2 or (o.threshold and 1 or 0)
   p.threshold = o.threshold or 0
   p.rectify = (o.rectify == 'image') and 1 or 0
   p.fix_mask_offset = o.fix_mask_offset and 1 or 0
   local t = p.tracker
   t.max_points, t.quality, t.min_dist = o.max_points or 400, o.points_quality or 1e-4, o.points_min_dist or 30   -- (:141 asks for 400 points)
   t.win, t.levels, t.max_iters, t.eps, t.min_eig, t.max_err = o.tracker_win_size or 21, 3, 30, 0.01, 1e-4, 0
   p.ransac_max_dist, p.iterations, p.seed = o.ransac2_max_dist or 1.0, 512, 0
   p.min_inlier_ratio = o.min_inlier_ratio or 0.2
   local h = ffi.new('dfe_stream*[1]')
   dfe.check(dfe.lib.dfe_stream_create(dfe.ctx, p, h))
   local n_img = g.hImg * g.wImg
   S = {h = h[0], p = p, keep = keep, layers = arr, C = p.C, H = p.Hsrc, W = p.Wsrc,
        frame = dfe.newBuffer(), ims = dfe.newBuffer(), flow = dfe.newBuffer(), mask = dfe.newBuffer(),
        im_scaled = torch.FloatTensor(p.C, g.hImg, g.wImg), output = torch.FloatTensor(2, g.hImg, g.wImg), maskt = torch.FloatTensor(g.hImg, g.wImg)}
   S.ims:reserve(p.C * n_img * 4); S.flow:reserve(2 * n_img * 4); S.mask:reserve(n_img * 4)
end

-- init{geometry =, filter =, K =, distP =, camera =, ...}: keeps the options; the stream is made when the first frame shows the camera's size.
-- The first frame is taken here, as the script's top level does (:69-72).
function M.init(opt)
   M.close()
   M.opt = opt
   if opt.camera then M.push(opt.camera:getNextFrame()) end
end

-- one frame -> status (0 first frame, 1 result, 2 bad image), im_scaled, output (2 x hImg x wImg: y, x), mask; M.last has R, T, nFound, nInliers
function M.push(frame)
   dfe.checktype(frame, 'torch.FloatTensor', 'depth_estimation_api: frame')
   if frame:nDimension() ~= 3 then error('depth_estimation_api: frame must be C x H x W') end
   if not S then open(frame) end
   if frame:size(1) ~= S.C or frame:size(2) ~= S.H or frame:size(3) ~= S.W then error('depth_estimation_api: the frame size changed') end
   local dframe = dfe.upload(frame, S.frame)
   local R, T = ffi.new('double[9]'), ffi.new('double[3]')
   local nf, ni, st = ffi.new('int[1]'), ffi.new('int[1]'), ffi.new('int[1]')
   dfe.check(dfe.lib.dfe_stream_push_f32(S.h, ffi.cast('const float*', dframe), 0, ffi.cast('float*', S.ims.ptr), ffi.cast('float*', S.flow.ptr),
                                         ffi.cast('float*', S.mask.ptr), nil, nil, R, T, nf, ni, st))
   dfe.download(S.im_scaled, S.ims.ptr)
   M.last = {status = st[0], nFound = nf[0], nInliers = ni[0], R = R, T = T}
   if st[0] ~= 0 then
      dfe.download(S.output, S.flow.ptr)
      dfe.download(S.maskt, S.mask.ptr)
   end
   return st[0], S.im_scaled, S.output, S.maskt
end

-- nextFrameDepth(): im_scaled, xflow, mask -- the three values the C++ caller reads (:196)
function M.nextFrameDepth()
   local st, im_scaled, output, mask = M.push(M.opt.camera:getNextFrame())
   if st == 0 then st, im_scaled, output, mask = M.push(M.opt.camera:getNextFrame()) end
   if st == 2 then print("BAD IMAGE !!! " .. M.last.nInliers .. " " .. M.last.nFound) end
   return im_scaled, output[2], mask
end

function M.reset()
   if S then dfe.check(dfe.lib.dfe_stream_reset(S.h)) end
end

function M.close()
   if S then
      dfe.lib.dfe_stream_destroy(S.h)
      for _, b in ipairs(S.keep) do b:free() end
      S.frame:free(); S.ims:free(); S.flow:free(); S.mask:free()
      S = nil
   end
end

return M
